// gnmixer.hip -- what the convolutional forks' blocks (model_sgm_mms_conv/model/HTR_VT.py and model_sgm_mms_conv_squeeze:
// ConvModule, FeedForward, SqueezeExcite1D, Downsample1D, Upsample1D) need beside the GEMM, LayerNorm and attention kernels,
// on token rows [B*N][C] as the GEMMs leave them (no transpose, no [B][C][N] copy).
//   htrvt_gnmixer_fwd         u [B*N][2C] -> c = dwconv(glu(u)) + bias, + per-workgroup partial pairs (sum c, sum c^2)
//   htrvt_gn_finalize         the pairs of one image, in order -> mean[b], rstd[b]  (GroupNorm(1, C): over all C * N values)
//   htrvt_gnmixer_act         s = silu((c - mean_b) * rstd_b * gamma + beta)
//   htrvt_gnmixer_bwd_reduce  dz = ds * silu'(z): partial rows per channel (sum dz, sum dz * xhat) and partial pairs per
//                             image (sum gamma dz, sum gamma dz xhat)
//   htrvt_gn_bwd_finalize     the pairs of one image -> m1[b], m2[b]
//   htrvt_gnmixer_bwd         dc = rstd_b * (gamma dz - m1_b - xhat m2_b) on the fly, convolved with the flipped taps, the GLU
//                             recomputed from u -> du; partial rows of d weight [C][k] and d bias [C]
//   htrvt_se_*                squeeze-excite gate: token means, the excite MLP per image in float32, y = x * g[b], and back
//   htrvt_seq_down2_*, htrvt_seq_up_add_*   pair averaging, nearest up-sampling fused with the skip add
//   htrvt_silu_fwd / _bwd     FeedForward's activation between its two GEMMs
// Work split of the mixer kernels: as in mixer.hip a thread owns one 16-byte channel vector and walks a run of `tl` tokens
// with a k-row register window, and a workgroup is cw channel vectors x 256 / cw runs -- but ALL runs of a workgroup belong
// to ONE image: blockIdx.x = b * wpi + wi, wpi = ceil(runs per image / runs per workgroup).  So every partial sum lies
// inside one image for every B, N and run length, the image's statistics are uniform over the workgroup, and the partials
// of image b are the consecutive entries b * P ... (b + 1) * P - 1, P = wpi * gridDim.y.  All sums are combined in a fixed
// order (registers -> LDS -> partial rows -> an ordered second stage): no float atomics, bitwise reproducible.
#include "rowvec.h"

using namespace htrvt;

namespace {

constexpr int NT = ROWVEC_NT;
constexpr int MAXK = 15;

inline int vec_len(int dtype) { return dtype == HTRVT_BF16 ? 8 : 4; }

// tl tokens per run, cw = 1 << lcw channel vectors per workgroup, wpi workgroups per image; grid (B * wpi, gy)
struct Split {
  int tl, lcw, gy, wpi;
  long long gx;
};

inline bool make_split(int B, int N, int C, int dtype, Split* s) {
  const int dv = C / vec_len(dtype);
  int lcw = 0;
  while ((1 << lcw) < dv && lcw < 5) ++lcw;
  if (dv > 32 && ((dv + 15) / 16) * 16 < ((dv + 31) / 32) * 32) lcw = 4;   // C = 384 bf16: 3 full groups of 16, not 32 + 16
  int tl = 16;   // shorter runs until the launch has three waves per SIMD (256 CUs x 4 SIMDs x 3 x 64 threads)
  while (tl > 4 && (long long)B * ((N + tl - 1) / tl) * dv < 196608) tl >>= 1;
  const int rpb = NT >> lcw;
  const int cpi = (N + tl - 1) / tl;
  s->tl = tl;
  s->lcw = lcw;
  s->wpi = (cpi + rpb - 1) / rpb;
  s->gy = (dv + (1 << lcw) - 1) >> lcw;
  s->gx = (long long)B * s->wpi;
  return s->gx <= 0x7fffffffLL && s->gy <= 65535 && s->gx * s->gy * NT < (1LL << 32);
}

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + __expf(-x)); }
__device__ __forceinline__ float silu_bwd(float ds, float z) {
  const float sg = sigmoid_f(z);
  return ds * sg * fmaf(z, 1.f - sg, 1.f);
}

// one thread's place: channel vector cv, image b, tokens [t0, t1); b is uniform over the workgroup
struct Place {
  int cv, cl, rl, b, t0, t1;
  bool active;
};
__device__ __forceinline__ Place my_place(int N, int dv, int tl, int lcw, int wpi) {
  Place p;
  p.cl = threadIdx.x & ((1 << lcw) - 1);
  p.rl = threadIdx.x >> lcw;
  p.cv = (blockIdx.y << lcw) + p.cl;
  p.b = blockIdx.x / wpi;
  const int run = (blockIdx.x % wpi) * (NT >> lcw) + p.rl;
  p.active = p.cv < dv && run < (N + tl - 1) / tl;
  p.t0 = p.active ? run * tl : 0;
  p.t1 = p.active ? min(N, p.t0 + tl) : 0;
  return p;
}

// the workgroup's pair (a, b) -> pairs[(blockIdx.x * gridDim.y + blockIdx.y) * 2 ...]: waves by shuffles, then the four waves
__device__ __forceinline__ void block_pair_out(float a, float b, float* red, float* __restrict__ pairs) {
  a = block_sum_256(a, red);
  b = block_sum_256(b, red + 4);
  if (threadIdx.x == 0) {
    float* o = pairs + ((long long)blockIdx.x * gridDim.y + blockIdx.y) * 2;
    o[0] = a;
    o[1] = b;
  }
}

// ------------------------------------------------------------------ mixer forward
template <typename T>
struct URow {
  Vec16<T> a, b;
  bool in;
};
template <typename T>
__device__ __forceinline__ URow<T> ld_urow(const T* __restrict__ u, long long base, int t, int N, int C, int c0) {
  URow<T> r;
  r.in = t >= 0 && t < N;
  if (r.in) {
    const long long o = (base + t) * 2 * C + c0;
    r.a = ld_vec(u, o);
    r.b = ld_vec(u, o + C);
  }
  return r;
}
template <typename T>
__device__ __forceinline__ void glu_row(const URow<T>& r, float (&g)[Vec16<T>::N]) {
#pragma unroll
  for (int e = 0; e < Vec16<T>::N; ++e) g[e] = r.in ? r.a.get(e) * sigmoid_f(r.b.get(e)) : 0.f;
}

// c = dwconv(glu(u)) + bias, rounded to T; the statistics are taken from the rounded values
template <typename T, int K>
__global__ __launch_bounds__(NT) void gnmixer_fwd_kernel(const T* __restrict__ u, const float* __restrict__ w,
                                                         const float* __restrict__ bias, T* __restrict__ cout,
                                                         float* __restrict__ pairs, int N, int C, int tl, int lcw, int wpi) {
  constexpr int CH = Vec16<T>::N, P = K / 2;
  __shared__ float red[8];
  const Place p = my_place(N, C / CH, tl, lcw, wpi);
  const int c0 = p.cv * CH;
  float s1 = 0.f, s2 = 0.f;
  if (p.active) {
    float wt[K][CH], bi[CH], win[K][CH];
#pragma unroll
    for (int e = 0; e < CH; ++e)
#pragma unroll
      for (int j = 0; j < K; ++j) wt[j][e] = w[(long long)(c0 + e) * K + j];
    ld_coef<CH>(bias, c0, 0.f, bi);
    const long long base = (long long)p.b * N;
#pragma unroll
    for (int i = 1; i < K; ++i) glu_row(ld_urow(u, base, p.t0 - P + i - 1, N, C, c0), win[i]);
    URow<T> nxt = ld_urow(u, base, p.t0 + P, N, C, c0);
    for (int n = p.t0; n < p.t1; ++n) {
      const URow<T> cur = nxt;
      if (n + 1 < p.t1) nxt = ld_urow(u, base, n + 1 + P, N, C, c0);     // the next row is in flight during this one
#pragma unroll
      for (int i = 0; i + 1 < K; ++i)
#pragma unroll
        for (int e = 0; e < CH; ++e) win[i][e] = win[i + 1][e];
      glu_row(cur, win[K - 1]);
      Vec16<T> cv;
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < K; ++j) a = fmaf(wt[j][e], win[j][e], a);
        const float cr = to_f32(from_f32<T>(a + bi[e]));
        cv.set(e, cr);
        s1 += cr;
        s2 = fmaf(cr, cr, s2);
      }
      st_vec(cout, (base + n) * C + c0, cv);
    }
  }
  block_pair_out(s1, s2, red, pairs);
}

// one thread per image: the P pairs of image b in order, in float64 (P is a handful; E[c^2] - mean^2 keeps its digits).
// BWD: (m1, m2) = the two sums / count.  Otherwise (mean, rstd) with the biased variance.
template <bool BWD>
__global__ __launch_bounds__(NT) void gn_finalize_kernel(const float* __restrict__ pairs, int B, int P, double count, float eps,
                                                         float* __restrict__ o0, float* __restrict__ o1) {
  const int b = blockIdx.x * NT + threadIdx.x;
  if (b >= B) return;
  double a = 0.0, q = 0.0;
  const float* p = pairs + (long long)b * P * 2;
  for (int i = 0; i < P; ++i) {
    a += (double)p[2 * i];
    q += (double)p[2 * i + 1];
  }
  a /= count;
  q /= count;
  if (BWD) {
    o0[b] = (float)a;
    o1[b] = (float)q;
  } else {
    const double var = fmax(q - a * a, 0.0);
    o0[b] = (float)a;
    o1[b] = (float)(1.0 / sqrt(var + (double)eps));
  }
}

// s = silu((c - mean_b) * rstd_b * gamma + beta); item = (row, channel vector), grid-stride
template <typename T>
__global__ __launch_bounds__(NT) void gnmixer_act_kernel(const T* __restrict__ c, const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, T* __restrict__ s, long long rows,
                                                         int N, int C) {
  constexpr int CH = Vec16<T>::N;
  const int dv = C / CH;
  const long long items = rows * dv, step = (long long)gridDim.x * NT;
  for (long long it = (long long)blockIdx.x * NT + threadIdx.x; it < items; it += step) {
    const long long r = it / dv;
    const int c0 = (int)(it - r * dv) * CH, b = (int)(r / N);
    float ga[CH], be[CH];
    ld_coef<CH>(gamma, c0, 1.f, ga);
    ld_coef<CH>(beta, c0, 0.f, be);
    const float mu = mean[b], rs = rstd[b];
    const Vec16<T> x = ld_vec(c, r * C + c0);
    Vec16<T> y;
#pragma unroll
    for (int e = 0; e < CH; ++e) {
      const float z = fmaf((x.get(e) - mu) * rs, ga[e], be[e]);
      y.set(e, z * sigmoid_f(z));
    }
    st_vec(s, r * C + c0, y);
  }
}

// ------------------------------------------------------------------ mixer backward
// pc[blockIdx.x][2][C] = (sum dz, sum dz * xhat) over the workgroup's runs, per channel; pi pair = (sum gamma dz, sum gamma dz xhat)
template <typename T>
__global__ __launch_bounds__(NT) void gnmixer_bwd_reduce_kernel(const T* __restrict__ ds, const T* __restrict__ c,
                                                                const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                float* __restrict__ pc, float* __restrict__ pi, int N, int C,
                                                                int tl, int lcw, int wpi) {
  constexpr int CH = Vec16<T>::N;
  __shared__ float red[NT * CH];
  const Place p = my_place(N, C / CH, tl, lcw, wpi);
  const int c0 = p.cv * CH;
  const bool col = p.cv < C / CH;
  float s1[CH], s2[CH], ga[CH];
#pragma unroll
  for (int e = 0; e < CH; ++e) s1[e] = s2[e] = ga[e] = 0.f;
  if (col) ld_coef<CH>(gamma, c0, 1.f, ga);
  if (p.active) {
    float be[CH];
    ld_coef<CH>(beta, c0, 0.f, be);
    const float mu = mean[p.b], rs = rstd[p.b];
    const long long base = (long long)p.b * N;
    for (int n = p.t0; n < p.t1; ++n) {
      const Vec16<T> dv = ld_vec(ds, (base + n) * C + c0), xv = ld_vec(c, (base + n) * C + c0);
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        const float xh = (xv.get(e) - mu) * rs;
        const float dz = silu_bwd(dv.get(e), fmaf(xh, ga[e], be[e]));
        s1[e] += dz;
        s2[e] = fmaf(dz, xh, s2[e]);
      }
    }
  }
  run_sum<CH>(s1, red, p.cl, p.rl, lcw);
  run_sum<CH>(s2, red, p.cl, p.rl, lcw);
  float t1 = 0.f, t2 = 0.f;
  if (p.rl == 0 && col) {
    float* row = pc + (long long)blockIdx.x * 2 * C + c0;
#pragma unroll
    for (int e = 0; e < CH; ++e) {
      row[e] = s1[e];
      row[C + e] = s2[e];
      t1 = fmaf(ga[e], s1[e], t1);
      t2 = fmaf(ga[e], s2[e], t2);
    }
  }
  __syncthreads();
  if (p.rl == 0) {
    red[2 * p.cl] = t1;
    red[2 * p.cl + 1] = t2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f, q = 0.f;
    for (int i = 0; i < (1 << lcw); ++i) {
      a += red[2 * i];
      q += red[2 * i + 1];
    }
    float* o = pi + ((long long)blockIdx.x * gridDim.y + blockIdx.y) * 2;
    o[0] = a;
    o[1] = q;
  }
}

template <typename T>
struct GRow {
  Vec16<T> ds, c;
  bool in;
};
template <typename T>
__device__ __forceinline__ GRow<T> ld_grow(const T* __restrict__ ds, const T* __restrict__ c, long long base, int t, int N, int C,
                                           int c0) {
  GRow<T> r;
  r.in = t >= 0 && t < N;
  if (r.in) {
    const long long o = (base + t) * C + c0;
    r.ds = ld_vec(ds, o);
    r.c = ld_vec(c, o);
  }
  return r;
}
// dc = rstd * (gamma dz - m1 - xhat m2) of a row (zero outside 0 .. N-1)
template <typename T>
__device__ __forceinline__ void dc_row(const GRow<T>& r, const float (&ga)[Vec16<T>::N], const float (&be)[Vec16<T>::N], float mu,
                                       float rs, float m1, float m2, float (&out)[Vec16<T>::N]) {
#pragma unroll
  for (int e = 0; e < Vec16<T>::N; ++e) {
    const float xh = r.in ? (r.c.get(e) - mu) * rs : 0.f;
    const float dz = silu_bwd(r.in ? r.ds.get(e) : 0.f, fmaf(xh, ga[e], be[e]));
    out[e] = r.in ? rs * (fmaf(ga[e], dz, -m1) - xh * m2) : 0.f;
  }
}

// du and the workgroup's partial rows pw [gridDim.x][C * K] (element c * K + j) and pb [gridDim.x][C].  With
// win[i] = dc(n + i - P):  dg(n) = sum_i w[K-1-i] * win[i]  and  d w[j] += g(n) * dc(n + P - j) = g(n) * win[K-1-j]
template <typename T, int K>
__global__ __launch_bounds__(NT) void gnmixer_bwd_kernel(const T* __restrict__ u, const T* __restrict__ c, const T* __restrict__ ds,
                                                         const float* __restrict__ w, const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, const float* __restrict__ m1v,
                                                         const float* __restrict__ m2v, T* __restrict__ du, float* __restrict__ pw,
                                                         float* __restrict__ pb, int N, int C, int tl, int lcw, int wpi) {
  constexpr int CH = Vec16<T>::N, P = K / 2;
  __shared__ float red[NT * CH];
  const Place p = my_place(N, C / CH, tl, lcw, wpi);
  const int c0 = p.cv * CH;
  float dw[K][CH], db[CH];
#pragma unroll
  for (int e = 0; e < CH; ++e) {
    db[e] = 0.f;
#pragma unroll
    for (int j = 0; j < K; ++j) dw[j][e] = 0.f;
  }
  if (p.active) {
    float wt[K][CH], ga[CH], be[CH], win[K][CH];
#pragma unroll
    for (int e = 0; e < CH; ++e)
#pragma unroll
      for (int j = 0; j < K; ++j) wt[j][e] = w[(long long)(c0 + e) * K + j];
    ld_coef<CH>(gamma, c0, 1.f, ga);
    ld_coef<CH>(beta, c0, 0.f, be);
    const float mu = mean[p.b], rs = rstd[p.b], m1 = m1v[p.b], m2 = m2v[p.b];
    const long long base = (long long)p.b * N;
#pragma unroll
    for (int i = 1; i < K; ++i) dc_row(ld_grow(ds, c, base, p.t0 - P + i - 1, N, C, c0), ga, be, mu, rs, m1, m2, win[i]);
    for (int n = p.t0; n < p.t1; ++n) {
      const GRow<T> gcur = ld_grow(ds, c, base, n + P, N, C, c0);
      const URow<T> ucur = ld_urow(u, base, n, N, C, c0);
#pragma unroll
      for (int i = 0; i + 1 < K; ++i)
#pragma unroll
        for (int e = 0; e < CH; ++e) win[i][e] = win[i + 1][e];
      dc_row(gcur, ga, be, mu, rs, m1, m2, win[K - 1]);
      const long long o = (base + n) * 2 * C + c0;
      Vec16<T> da, dbv;
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        float dg = 0.f;
#pragma unroll
        for (int i = 0; i < K; ++i) dg = fmaf(wt[K - 1 - i][e], win[i][e], dg);
        const float av = ucur.a.get(e), sg = sigmoid_f(ucur.b.get(e));
        const float g = av * sg;
#pragma unroll
        for (int j = 0; j < K; ++j) dw[j][e] = fmaf(g, win[K - 1 - j][e], dw[j][e]);
        db[e] += win[P][e];
        da.set(e, dg * sg);
        dbv.set(e, dg * g * (1.f - sg));
      }
      st_vec(du, o, da);
      st_vec(du, o + C, dbv);
    }
  }
  const bool writer = p.rl == 0 && p.cv < C / CH;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    run_sum<CH>(dw[j], red, p.cl, p.rl, lcw);
    if (writer) {
      float* row = pw + (long long)blockIdx.x * C * K;
#pragma unroll
      for (int e = 0; e < CH; ++e) row[(long long)(c0 + e) * K + j] = dw[j][e];
    }
  }
  run_sum<CH>(db, red, p.cl, p.rl, lcw);
  if (writer) {
#pragma unroll
    for (int e = 0; e < CH; ++e) pb[(long long)blockIdx.x * C + c0 + e] = db[e];
  }
}

// ------------------------------------------------------------------ squeeze-excite
// out[b][d] = scale * sum_n x[b][n][d] (* y[b][n][d] where y != NULL): grid (B, channel groups); a thread takes the tokens
// rl, rl + rpb, ... of its channel vector, the runs are added in the order of rl
template <typename T>
__global__ __launch_bounds__(NT) void se_reduce_kernel(const T* __restrict__ x, const T* __restrict__ y, float* __restrict__ out,
                                                       int N, int D, float scale, int lcw) {
  constexpr int CH = Vec16<T>::N;
  __shared__ float red[NT * CH];
  const int cl = threadIdx.x & ((1 << lcw) - 1), rl = threadIdx.x >> lcw, rpb = NT >> lcw;
  const int cv = (blockIdx.y << lcw) + cl, c0 = cv * CH;
  const bool col = cv < D / CH;
  float acc[CH];
#pragma unroll
  for (int e = 0; e < CH; ++e) acc[e] = 0.f;
  if (col) {
    const long long base = (long long)blockIdx.x * N;
    for (int n = rl; n < N; n += rpb) {
      const Vec16<T> xv = ld_vec(x, (base + n) * D + c0);
      if (y) {
        const Vec16<T> yv = ld_vec(y, (base + n) * D + c0);
#pragma unroll
        for (int e = 0; e < CH; ++e) acc[e] = fmaf(xv.get(e), yv.get(e), acc[e]);
      } else {
#pragma unroll
        for (int e = 0; e < CH; ++e) acc[e] += xv.get(e);
      }
    }
  }
  run_sum<CH>(acc, red, cl, rl, lcw);
  if (rl == 0 && col) {
#pragma unroll
    for (int e = 0; e < CH; ++e) out[(long long)blockIdx.x * D + c0 + e] = acc[e] * scale;
  }
}

// out = x * g[b] (+ add[b] * addscale where add != NULL)
template <typename T>
__global__ __launch_bounds__(NT) void se_scale_kernel(const T* __restrict__ x, const float* __restrict__ g,
                                                      const float* __restrict__ add, float addscale, T* __restrict__ out,
                                                      long long rows, int N, int D) {
  constexpr int CH = Vec16<T>::N;
  const int dv = D / CH;
  const long long items = rows * dv, step = (long long)gridDim.x * NT;
  for (long long it = (long long)blockIdx.x * NT + threadIdx.x; it < items; it += step) {
    const long long r = it / dv;
    const int c0 = (int)(it - r * dv) * CH;
    const long long gb = (r / N) * D;
    float gv[CH], av[CH];
    ld_coef<CH>(g + gb, c0, 1.f, gv);
    ld_coef<CH>(add ? add + gb : nullptr, c0, 0.f, av);
    const Vec16<T> xv = ld_vec(x, r * D + c0);
    Vec16<T> y;
#pragma unroll
    for (int e = 0; e < CH; ++e) y.set(e, fmaf(xv.get(e), gv[e], av[e] * addscale));
    st_vec(out, r * D + c0, y);
  }
}

__device__ __forceinline__ float sigmoid_precise(float x) { return 1.0f / (1.0f + expf(-x)); }

// The excite MLP runs one workgroup of 16 waves per image; its weights (0.6 MB each at D = 768) come from the L2, and what
// bounds a workgroup is the latency of those loads, so every wave keeps several rows in flight.
constexpr int MLP_NT = 1024, MLP_NW = MLP_NT / 64;

// out(o) = sum_i W[o][i] * v[i], o < No, i < K (v in LDS, 16-byte aligned): a wave per output, lanes over i, eight outputs
// in flight per wave; 16-byte loads where the rows allow
template <typename F>
__device__ __forceinline__ void row_dots(const float* __restrict__ W, const float* v, int K, int No, F&& emit) {
  constexpr int U = 8;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const bool vec = (K & 3) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0;
  for (int o0 = wv * U; o0 < No; o0 += MLP_NW * U) {
    float a[U];
#pragma unroll
    for (int q = 0; q < U; ++q) a[q] = 0.f;
    if (vec) {
      for (int i = lane * 4; i < K; i += 256) {
        const float4 x = *reinterpret_cast<const float4*>(v + i);
#pragma unroll
        for (int q = 0; q < U; ++q)
          if (o0 + q < No) {
            const float4 t = *reinterpret_cast<const float4*>(W + (long long)(o0 + q) * K + i);
            a[q] = fmaf(t.w, x.w, fmaf(t.z, x.z, fmaf(t.y, x.y, fmaf(t.x, x.x, a[q]))));
          }
      }
    } else {
      for (int i = lane; i < K; i += 64) {
        const float x = v[i];
#pragma unroll
        for (int q = 0; q < U; ++q)
          if (o0 + q < No) a[q] = fmaf(W[(long long)(o0 + q) * K + i], x, a[q]);
      }
    }
#pragma unroll
    for (int q = 0; q < U; ++q) {
      const float t = wave_sum(a[q]);
      if (lane == 0 && o0 + q < No) emit(o0 + q, t);
    }
  }
}

// out[o] = sum_i v[i] * W[i][o], o < No, i < Ni (v in LDS, W's rows of length No): 64 outputs per pass, lanes over o, the i
// range dealt over the 16 waves, whose partials (part: LDS [16][64]) are added in the order of the waves
__device__ __forceinline__ void col_dots(const float* __restrict__ W, const float* v, int Ni, int No, float* part, float* out) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int o0 = 0; o0 < No; o0 += 64) {
    const int o = o0 + lane;
    float a = 0.f;
    if (o < No) {
#pragma unroll 4
      for (int i = wv; i < Ni; i += MLP_NW) a = fmaf(v[i], W[(long long)i * No + o], a);
    }
    part[wv * 64 + lane] = a;
    __syncthreads();
    if (wv == 0 && o < No) {
      float t = 0.f;
      for (int w = 0; w < MLP_NW; ++w) t += part[w * 64 + lane];
      out[o] = t;
    }
    __syncthreads();
  }
}

// one workgroup per image: pre = fc1(mean), act = silu(pre), g = sigmoid(fc2(act))
__global__ __launch_bounds__(MLP_NT) void se_mlp_fwd_kernel(const float* __restrict__ mean, const float* __restrict__ w1,
                                                            const float* __restrict__ b1, const float* __restrict__ w2,
                                                            const float* __restrict__ b2, float* __restrict__ pre,
                                                            float* __restrict__ act, float* __restrict__ g, int D, int H) {
  extern __shared__ float sm[];
  float* xs = sm;
  float* as = sm + D;
  const long long b = blockIdx.x;
  for (int d = threadIdx.x; d < D; d += MLP_NT) xs[d] = mean[b * D + d];
  __syncthreads();
  row_dots(w1, xs, D, H, [&](int j, float t) {
    const float h = t + b1[j], s = h * sigmoid_precise(h);
    pre[b * H + j] = h;
    act[b * H + j] = s;
    as[j] = s;
  });
  __syncthreads();
  row_dots(w2, as, H, D, [&](int d, float t) { g[b * D + d] = sigmoid_precise(t + b2[d]); });
}

// one workgroup per image: dh2 = dg * g (1 - g), dh1 = (dh2 fc2) * silu'(pre), dmean = dh1 fc1
__global__ __launch_bounds__(MLP_NT) void se_mlp_bwd_kernel(const float* __restrict__ dg, const float* __restrict__ g,
                                                            const float* __restrict__ pre, const float* __restrict__ w1,
                                                            const float* __restrict__ w2, float* __restrict__ dh2,
                                                            float* __restrict__ dh1, float* __restrict__ dmean, int D, int H) {
  extern __shared__ float sm[];
  __shared__ float part[MLP_NW * 64];
  float* d2 = sm;
  float* d1 = sm + D;
  const long long b = blockIdx.x;
  for (int d = threadIdx.x; d < D; d += MLP_NT) {
    const float gv = g[b * D + d], v = dg[b * D + d] * gv * (1.f - gv);
    d2[d] = v;
    dh2[b * D + d] = v;
  }
  __syncthreads();
  col_dots(w2, d2, D, H, part, d1);
  for (int j = threadIdx.x; j < H; j += MLP_NT) {
    const float h = pre[b * H + j], sg = sigmoid_precise(h);
    const float v = d1[j] * sg * fmaf(h, 1.f - sg, 1.f);
    d1[j] = v;
    dh1[b * H + j] = v;
  }
  __syncthreads();
  col_dots(w1, d1, H, D, part, dmean + b * D);
}

// dw[m][k] = sum_b dy[b][m] * x[b][k], db[m] = sum_b dy[b][m], b in increasing order
__global__ __launch_bounds__(NT) void se_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                      float* __restrict__ dw, float* __restrict__ db, int B, int M, int K) {
  const long long items = (long long)M * K, step = (long long)gridDim.x * NT;
  for (long long it = (long long)blockIdx.x * NT + threadIdx.x; it < items; it += step) {
    const int m = (int)(it / K), k = (int)(it - (long long)m * K);
    float a = 0.f, s = 0.f;
    for (int b = 0; b < B; ++b) {
      const float d = dy[(long long)b * M + m];
      a = fmaf(d, x[(long long)b * K + k], a);
      s += d;
    }
    dw[it] = a;
    if (k == 0) db[m] = s;
  }
}

// ------------------------------------------------------------------ resampling and SiLU; item = (output row, channel vector)
enum { OP_DOWN_FWD, OP_DOWN_BWD, OP_UP_FWD, OP_UP_BWD };

// n: tokens of the short sequence, N: tokens of the long one; a: the first input, b: the skip rows of OP_UP_FWD
template <typename T, int OP>
__global__ __launch_bounds__(NT) void resample_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ out,
                                                      int B, int n, int N, int D) {
  constexpr int CH = Vec16<T>::N;
  const int dv = D / CH;
  const int To = (OP == OP_DOWN_FWD || OP == OP_UP_BWD) ? n : N;      // tokens per image of the output
  const long long items = (long long)B * To * dv, step = (long long)gridDim.x * NT;
  for (long long it = (long long)blockIdx.x * NT + threadIdx.x; it < items; it += step) {
    const long long r = it / dv;
    const int c0 = (int)(it - r * dv) * CH;
    const long long img = r / To;
    const int t = (int)(r - img * To);
    float acc[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) acc[e] = 0.f;
    if (OP == OP_DOWN_FWD) {
      const Vec16<T> x0 = ld_vec(a, (img * N + 2 * t) * D + c0), x1 = ld_vec(a, (img * N + 2 * t + 1) * D + c0);
#pragma unroll
      for (int e = 0; e < CH; ++e) acc[e] = 0.5f * (x0.get(e) + x1.get(e));
    } else if (OP == OP_DOWN_BWD) {
      if (t < 2 * n) {
        const Vec16<T> d = ld_vec(a, (img * n + (t >> 1)) * D + c0);
#pragma unroll
        for (int e = 0; e < CH; ++e) acc[e] = 0.5f * d.get(e);
      }
    } else if (OP == OP_UP_FWD) {
      const int src = (int)(((long long)t * n) / N);
      const Vec16<T> y = ld_vec(a, (img * n + src) * D + c0), sk = ld_vec(b, r * D + c0);
#pragma unroll
      for (int e = 0; e < CH; ++e) acc[e] = y.get(e) + sk.get(e);
    } else {
      // the targets i of source t: (i n) / N == t  <=>  ceil(t N / n) <= i < ceil((t + 1) N / n)
      const int lo = (int)(((long long)t * N + n - 1) / n), hi = (int)((((long long)t + 1) * N + n - 1) / n);
      for (int i = lo; i < hi && i < N; ++i) {
        const Vec16<T> d = ld_vec(a, (img * N + i) * D + c0);
#pragma unroll
        for (int e = 0; e < CH; ++e) acc[e] += d.get(e);
      }
    }
    Vec16<T> o;
#pragma unroll
    for (int e = 0; e < CH; ++e) o.set(e, acc[e]);
    st_vec(out, r * D + c0, o);
  }
}

// BWD: out = da * silu'(pre); otherwise out = silu(pre)
template <typename T, bool BWD>
__global__ __launch_bounds__(NT) void silu_kernel(const T* __restrict__ pre, const T* __restrict__ da, T* __restrict__ out,
                                                  long long nvec) {
  constexpr int CH = Vec16<T>::N;
  const long long step = (long long)gridDim.x * NT;
  for (long long it = (long long)blockIdx.x * NT + threadIdx.x; it < nvec; it += step) {
    const Vec16<T> x = ld_vec(pre, it * CH);
    Vec16<T> d, y;
    if (BWD) d = ld_vec(da, it * CH);
#pragma unroll
    for (int e = 0; e < CH; ++e) {
      const float z = x.get(e);
      y.set(e, BWD ? silu_bwd(d.get(e), z) : z * sigmoid_f(z));
    }
    st_vec(out, it * CH, y);
  }
}

// ------------------------------------------------------------------ host side
inline unsigned flat_blocks(long long items) {
  const long long g = (items + NT - 1) / NT;
  return (unsigned)(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

int check_rows(const char* what, int B, int N, int D, int dtype) {
  HTRVT_REQUIRE(dtype == HTRVT_F32 || dtype == HTRVT_BF16, "%s: dtype %d", what, dtype);
  HTRVT_REQUIRE(B >= 1 && N >= 1 && D >= 1, "%s: B=%d N=%d D=%d", what, B, N, D);
  HTRVT_REQUIRE(D % vec_len(dtype) == 0, "%s: D=%d is not a multiple of the 16-byte vector (%d elements)", what, D, vec_len(dtype));
  HTRVT_REQUIRE((long long)B * N < (1ll << 31), "%s: too many rows", what);
  return 0;
}

int check_mixer(const char* what, int B, int N, int C, int k, int dtype, Split* sp) {
  if (check_rows(what, B, N, C, dtype)) return -1;
  HTRVT_REQUIRE(k >= 1 && k <= MAXK && (k & 1), "%s: kernel size %d (odd, 1 ... %d)", what, k, MAXK);
  HTRVT_REQUIRE(make_split(B, N, C, dtype, sp), "%s: B=%d N=%d C=%d does not fit one launch", what, B, N, C);
  return 0;
}

int lcw_of(int D, int dtype) {
  const int dv = D / vec_len(dtype);
  int lcw = 0;
  while ((1 << lcw) < dv && lcw < 5) ++lcw;
  return lcw;
}

#define GN_BY_K(k, LAUNCH)      \
  switch (k) {                  \
    case 1: LAUNCH(1); break;   \
    case 3: LAUNCH(3); break;   \
    case 5: LAUNCH(5); break;   \
    case 7: LAUNCH(7); break;   \
    case 9: LAUNCH(9); break;   \
    case 11: LAUNCH(11); break; \
    case 13: LAUNCH(13); break; \
    default: LAUNCH(15); break; \
  }

template <typename T>
void launch_fwd(const Split& sp, hipStream_t st, int k, const void* u, const float* w, const float* bias, void* c, float* pairs,
                int N, int C) {
  const dim3 grid((unsigned)sp.gx, sp.gy);
#define LAUNCH(KK)                                                                                                        \
  hipLaunchKernelGGL((gnmixer_fwd_kernel<T, KK>), grid, dim3(NT), 0, st, (const T*)u, w, bias, (T*)c, pairs, N, C, sp.tl, \
                     sp.lcw, sp.wpi)
  GN_BY_K(k, LAUNCH)
#undef LAUNCH
}

template <typename T>
void launch_bwd(const Split& sp, hipStream_t st, int k, const void* u, const void* c, const void* ds, const float* w,
                const float* mean, const float* rstd, const float* gamma, const float* beta, const float* m1, const float* m2,
                void* du, float* pw, float* pb, int N, int C) {
  const dim3 grid((unsigned)sp.gx, sp.gy);
#define LAUNCH(KK)                                                                                                          \
  hipLaunchKernelGGL((gnmixer_bwd_kernel<T, KK>), grid, dim3(NT), 0, st, (const T*)u, (const T*)c, (const T*)ds, w, mean, \
                     rstd, gamma, beta, m1, m2, (T*)du, pw, pb, N, C, sp.tl, sp.lcw, sp.wpi)
  GN_BY_K(k, LAUNCH)
#undef LAUNCH
}

template <bool BWD>
int finalize(const char* what, const float* pairs, int B, int P, double count, float eps, float* o0, float* o1, void* stream) {
  HTRVT_REQUIRE(B >= 1 && P >= 1 && count >= 1.0, "%s: B=%d P=%d count=%g", what, B, P, count);
  HTRVT_REQUIRE(pairs && o0 && o1, "%s: null buffer", what);
  hipLaunchKernelGGL(gn_finalize_kernel<BWD>, dim3((B + NT - 1) / NT), dim3(NT), 0, (hipStream_t)stream, pairs, B, P, count, eps,
                     o0, o1);
  return check_launch(what);
}

template <int OP>
int resample(const char* what, const void* a, const void* b, void* out, int B, int n, int N, int D, int dtype, void* stream) {
  if (check_rows(what, B, N, D, dtype)) return -1;
  HTRVT_REQUIRE(n >= 1 && n <= N, "%s: n=%d of N=%d tokens", what, n, N);
  HTRVT_REQUIRE(a && out && (OP != OP_UP_FWD || b), "%s: null buffer", what);
  HTRVT_REQUIRE(!misaligned16(a, b, out), "%s: buffers not 16-byte aligned", what);
  const int To = (OP == OP_DOWN_FWD || OP == OP_UP_BWD) ? n : N;
  const dim3 grid(flat_blocks((long long)B * To * (D / vec_len(dtype))));
  if (dtype == HTRVT_BF16)
    hipLaunchKernelGGL((resample_kernel<bf16_t, OP>), grid, dim3(NT), 0, (hipStream_t)stream, (const bf16_t*)a, (const bf16_t*)b,
                       (bf16_t*)out, B, n, N, D);
  else
    hipLaunchKernelGGL((resample_kernel<float, OP>), grid, dim3(NT), 0, (hipStream_t)stream, (const float*)a, (const float*)b,
                       (float*)out, B, n, N, D);
  return check_launch(what);
}

}  // namespace

extern "C" int htrvt_gnmixer_rows(int B, int N, int C, int dtype) {
  Split sp;
  if (check_mixer("htrvt_gnmixer_rows", B, N, C, 1, dtype, &sp)) return -1;
  return (int)sp.gx;
}

extern "C" int htrvt_gnmixer_parts(int B, int N, int C, int dtype) {
  Split sp;
  if (check_mixer("htrvt_gnmixer_parts", B, N, C, 1, dtype, &sp)) return -1;
  return sp.wpi * sp.gy;
}

extern "C" int htrvt_gnmixer_fwd(const void* u, const float* w, const float* bias, void* c, float* pairs, int B, int N, int C,
                                 int k, int dtype, void* stream) {
  Split sp;
  if (check_mixer("htrvt_gnmixer_fwd", B, N, C, k, dtype, &sp)) return -1;
  HTRVT_REQUIRE(u && w && c && pairs, "htrvt_gnmixer_fwd: null buffer");
  HTRVT_REQUIRE(!misaligned16(u, c), "htrvt_gnmixer_fwd: u / c not 16-byte aligned");
  if (dtype == HTRVT_BF16)
    launch_fwd<bf16_t>(sp, (hipStream_t)stream, k, u, w, bias, c, pairs, N, C);
  else
    launch_fwd<float>(sp, (hipStream_t)stream, k, u, w, bias, c, pairs, N, C);
  return check_launch("gnmixer_fwd");
}

extern "C" int htrvt_gn_finalize(const float* pairs, int B, int P, double count, float eps, float* mean, float* rstd,
                                 void* stream) {
  return finalize<false>("htrvt_gn_finalize", pairs, B, P, count, eps, mean, rstd, stream);
}

extern "C" int htrvt_gn_bwd_finalize(const float* pairs, int B, int P, double count, float* m1, float* m2, void* stream) {
  return finalize<true>("htrvt_gn_bwd_finalize", pairs, B, P, count, 0.f, m1, m2, stream);
}

extern "C" int htrvt_gnmixer_act(const void* c, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                 void* s, int B, int N, int C, int dtype, void* stream) {
  if (check_rows("htrvt_gnmixer_act", B, N, C, dtype)) return -1;
  HTRVT_REQUIRE(c && mean && rstd && s, "htrvt_gnmixer_act: null buffer");
  HTRVT_REQUIRE(!misaligned16(c, s), "htrvt_gnmixer_act: c / s not 16-byte aligned");
  const long long rows = (long long)B * N;
  const dim3 grid(flat_blocks(rows * (C / vec_len(dtype))));
  if (dtype == HTRVT_BF16)
    hipLaunchKernelGGL(gnmixer_act_kernel<bf16_t>, grid, dim3(NT), 0, (hipStream_t)stream, (const bf16_t*)c, mean, rstd, gamma,
                       beta, (bf16_t*)s, rows, N, C);
  else
    hipLaunchKernelGGL(gnmixer_act_kernel<float>, grid, dim3(NT), 0, (hipStream_t)stream, (const float*)c, mean, rstd, gamma,
                       beta, (float*)s, rows, N, C);
  return check_launch("gnmixer_act");
}

extern "C" int htrvt_gnmixer_bwd_reduce(const void* ds, const void* c, const float* mean, const float* rstd, const float* gamma,
                                        const float* beta, float* chan_partial, float* pairs, int B, int N, int C, int dtype,
                                        void* stream) {
  Split sp;
  if (check_mixer("htrvt_gnmixer_bwd_reduce", B, N, C, 1, dtype, &sp)) return -1;
  HTRVT_REQUIRE(ds && c && mean && rstd && chan_partial && pairs, "htrvt_gnmixer_bwd_reduce: null buffer");
  HTRVT_REQUIRE(!misaligned16(ds, c), "htrvt_gnmixer_bwd_reduce: ds / c not 16-byte aligned");
  const dim3 grid((unsigned)sp.gx, sp.gy);
  if (dtype == HTRVT_BF16)
    hipLaunchKernelGGL(gnmixer_bwd_reduce_kernel<bf16_t>, grid, dim3(NT), 0, (hipStream_t)stream, (const bf16_t*)ds,
                       (const bf16_t*)c, mean, rstd, gamma, beta, chan_partial, pairs, N, C, sp.tl, sp.lcw, sp.wpi);
  else
    hipLaunchKernelGGL(gnmixer_bwd_reduce_kernel<float>, grid, dim3(NT), 0, (hipStream_t)stream, (const float*)ds,
                       (const float*)c, mean, rstd, gamma, beta, chan_partial, pairs, N, C, sp.tl, sp.lcw, sp.wpi);
  return check_launch("gnmixer_bwd_reduce");
}

extern "C" int htrvt_gnmixer_bwd(const void* u, const void* c, const void* ds, const float* w, const float* mean,
                                 const float* rstd, const float* gamma, const float* beta, const float* m1, const float* m2,
                                 void* du, float* dw_partial, float* db_partial, int B, int N, int C, int k, int dtype,
                                 void* stream) {
  Split sp;
  if (check_mixer("htrvt_gnmixer_bwd", B, N, C, k, dtype, &sp)) return -1;
  HTRVT_REQUIRE(u && c && ds && w && mean && rstd && m1 && m2 && du && dw_partial && db_partial, "htrvt_gnmixer_bwd: null buffer");
  HTRVT_REQUIRE(!misaligned16(u, c, ds, du), "htrvt_gnmixer_bwd: u / c / ds / du not 16-byte aligned");
  if (dtype == HTRVT_BF16)
    launch_bwd<bf16_t>(sp, (hipStream_t)stream, k, u, c, ds, w, mean, rstd, gamma, beta, m1, m2, du, dw_partial, db_partial, N, C);
  else
    launch_bwd<float>(sp, (hipStream_t)stream, k, u, c, ds, w, mean, rstd, gamma, beta, m1, m2, du, dw_partial, db_partial, N, C);
  return check_launch("gnmixer_bwd");
}

// ---- squeeze-excite
static int se_reduce(const char* what, const void* x, const void* y, float* out, int B, int N, int D, float scale, int dtype,
                     void* stream) {
  if (check_rows(what, B, N, D, dtype)) return -1;
  HTRVT_REQUIRE(x && out, "%s: null buffer", what);
  HTRVT_REQUIRE(!misaligned16(x, y), "%s: inputs not 16-byte aligned", what);
  const int lcw = lcw_of(D, dtype), dv = D / vec_len(dtype);
  const int gy = (dv + (1 << lcw) - 1) >> lcw;
  HTRVT_REQUIRE(gy <= 65535 && (long long)B * gy * NT < (1LL << 32), "%s: B=%d D=%d does not fit one launch", what, B, D);
  const dim3 grid(B, gy);
  if (dtype == HTRVT_BF16)
    hipLaunchKernelGGL(se_reduce_kernel<bf16_t>, grid, dim3(NT), 0, (hipStream_t)stream, (const bf16_t*)x, (const bf16_t*)y, out,
                       N, D, scale, lcw);
  else
    hipLaunchKernelGGL(se_reduce_kernel<float>, grid, dim3(NT), 0, (hipStream_t)stream, (const float*)x, (const float*)y, out, N,
                       D, scale, lcw);
  return check_launch(what);
}

static int se_scale(const char* what, const void* x, const float* g, const float* add, float addscale, void* out, int B, int N,
                    int D, int dtype, void* stream) {
  if (check_rows(what, B, N, D, dtype)) return -1;
  HTRVT_REQUIRE(x && g && out, "%s: null buffer", what);
  HTRVT_REQUIRE(!misaligned16(x, out), "%s: x / out not 16-byte aligned", what);
  const long long rows = (long long)B * N;
  const dim3 grid(flat_blocks(rows * (D / vec_len(dtype))));
  if (dtype == HTRVT_BF16)
    hipLaunchKernelGGL(se_scale_kernel<bf16_t>, grid, dim3(NT), 0, (hipStream_t)stream, (const bf16_t*)x, g, add, addscale,
                       (bf16_t*)out, rows, N, D);
  else
    hipLaunchKernelGGL(se_scale_kernel<float>, grid, dim3(NT), 0, (hipStream_t)stream, (const float*)x, g, add, addscale,
                       (float*)out, rows, N, D);
  return check_launch(what);
}

extern "C" int htrvt_se_mean(const void* x, float* mean, int B, int N, int D, int dtype, void* stream) {
  return se_reduce("htrvt_se_mean", x, nullptr, mean, B, N, D, 1.0f / (float)N, dtype, stream);
}

extern "C" int htrvt_se_scale_fwd(const void* x, const float* g, void* y, int B, int N, int D, int dtype, void* stream) {
  return se_scale("htrvt_se_scale_fwd", x, g, nullptr, 0.f, y, B, N, D, dtype, stream);
}

extern "C" int htrvt_se_scale_bwd_reduce(const void* dy, const void* x, float* dg, int B, int N, int D, int dtype, void* stream) {
  HTRVT_REQUIRE(x, "htrvt_se_scale_bwd_reduce: null buffer");
  return se_reduce("htrvt_se_scale_bwd_reduce", dy, x, dg, B, N, D, 1.0f, dtype, stream);
}

extern "C" int htrvt_se_scale_bwd(const void* dy, const float* g, const float* dmean, void* dx, int B, int N, int D, int dtype,
                                  void* stream) {
  HTRVT_REQUIRE(dmean, "htrvt_se_scale_bwd: null buffer");
  return se_scale("htrvt_se_scale_bwd", dy, g, dmean, 1.0f / (float)N, dx, B, N, D, dtype, stream);
}

static int check_mlp(const char* what, int B, int D, int H) {
  HTRVT_REQUIRE(B >= 1 && D >= 1 && H >= 1, "%s: B=%d D=%d hidden=%d", what, B, D, H);
  HTRVT_REQUIRE((long long)D + H <= 16384, "%s: D + hidden = %d floats do not fit the LDS", what, D + H);
  return 0;
}

extern "C" int htrvt_se_mlp_fwd(const float* mean, const float* w1, const float* b1, const float* w2, const float* b2, float* pre,
                                float* act, float* g, int B, int D, int H, void* stream) {
  if (check_mlp("htrvt_se_mlp_fwd", B, D, H)) return -1;
  HTRVT_REQUIRE(mean && w1 && b1 && w2 && b2 && pre && act && g, "htrvt_se_mlp_fwd: null buffer");
  hipLaunchKernelGGL(se_mlp_fwd_kernel, dim3(B), dim3(MLP_NT), (size_t)(D + H) * 4, (hipStream_t)stream, mean, w1, b1, w2, b2, pre,
                     act, g, D, H);
  return check_launch("se_mlp_fwd");
}

extern "C" int htrvt_se_mlp_bwd(const float* dg, const float* g, const float* pre, const float* w1, const float* w2, float* dh2,
                                float* dh1, float* dmean, int B, int D, int H, void* stream) {
  if (check_mlp("htrvt_se_mlp_bwd", B, D, H)) return -1;
  HTRVT_REQUIRE(dg && g && pre && w1 && w2 && dh2 && dh1 && dmean, "htrvt_se_mlp_bwd: null buffer");
  hipLaunchKernelGGL(se_mlp_bwd_kernel, dim3(B), dim3(MLP_NT), (size_t)(D + H) * 4, (hipStream_t)stream, dg, g, pre, w1, w2, dh2, dh1,
                     dmean, D, H);
  return check_launch("se_mlp_bwd");
}

extern "C" int htrvt_se_wgrad(const float* dy, const float* x, float* dw, float* db, int B, int M, int K, void* stream) {
  HTRVT_REQUIRE(B >= 1 && M >= 1 && K >= 1, "htrvt_se_wgrad: B=%d M=%d K=%d", B, M, K);
  HTRVT_REQUIRE(dy && x && dw && db, "htrvt_se_wgrad: null buffer");
  hipLaunchKernelGGL(se_wgrad_kernel, dim3(flat_blocks((long long)M * K)), dim3(NT), 0, (hipStream_t)stream, dy, x, dw, db, B, M,
                     K);
  return check_launch("se_wgrad");
}

// ---- resampling
extern "C" int htrvt_seq_down2_fwd(const void* x, void* y, int B, int N, int D, int dtype, void* stream) {
  HTRVT_REQUIRE(N >= 2, "htrvt_seq_down2_fwd: N=%d (N <= 1 is the identity: no launch)", N);
  return resample<OP_DOWN_FWD>("htrvt_seq_down2_fwd", x, nullptr, y, B, N / 2, N, D, dtype, stream);
}

extern "C" int htrvt_seq_down2_bwd(const void* dy, void* dx, int B, int N, int D, int dtype, void* stream) {
  HTRVT_REQUIRE(N >= 2, "htrvt_seq_down2_bwd: N=%d (N <= 1 is the identity: no launch)", N);
  return resample<OP_DOWN_BWD>("htrvt_seq_down2_bwd", dy, nullptr, dx, B, N / 2, N, D, dtype, stream);
}

extern "C" int htrvt_seq_up_add_fwd(const void* y, const void* skip, void* out, int B, int n, int N0, int D, int dtype,
                                    void* stream) {
  return resample<OP_UP_FWD>("htrvt_seq_up_add_fwd", y, skip, out, B, n, N0, D, dtype, stream);
}

extern "C" int htrvt_seq_up_add_bwd(const void* dout, void* dy, int B, int n, int N0, int D, int dtype, void* stream) {
  return resample<OP_UP_BWD>("htrvt_seq_up_add_bwd", dout, nullptr, dy, B, n, N0, D, dtype, stream);
}

// ---- SiLU
static int silu(const char* what, const void* pre, const void* da, void* out, int64_t n, int dtype, bool bwd, void* stream) {
  HTRVT_REQUIRE(dtype == HTRVT_F32 || dtype == HTRVT_BF16, "%s: dtype %d", what, dtype);
  HTRVT_REQUIRE(n >= 0 && n % vec_len(dtype) == 0, "%s: n=%lld is not a multiple of the 16-byte vector (%d elements)", what,
                (long long)n, vec_len(dtype));
  if (n == 0) return 0;
  HTRVT_REQUIRE(pre && out && (!bwd || da), "%s: null buffer", what);
  HTRVT_REQUIRE(!misaligned16(pre, da, out), "%s: buffers not 16-byte aligned", what);
  const long long nvec = n / vec_len(dtype);
  const dim3 grid(flat_blocks(nvec));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == HTRVT_BF16) {
    if (bwd)
      hipLaunchKernelGGL((silu_kernel<bf16_t, true>), grid, dim3(NT), 0, st, (const bf16_t*)pre, (const bf16_t*)da, (bf16_t*)out, nvec);
    else
      hipLaunchKernelGGL((silu_kernel<bf16_t, false>), grid, dim3(NT), 0, st, (const bf16_t*)pre, (const bf16_t*)da, (bf16_t*)out, nvec);
  } else {
    if (bwd)
      hipLaunchKernelGGL((silu_kernel<float, true>), grid, dim3(NT), 0, st, (const float*)pre, (const float*)da, (float*)out, nvec);
    else
      hipLaunchKernelGGL((silu_kernel<float, false>), grid, dim3(NT), 0, st, (const float*)pre, (const float*)da, (float*)out, nvec);
  }
  return check_launch(what);
}

extern "C" int htrvt_silu_fwd(const void* pre, void* a, int64_t n, int dtype, void* stream) {
  return silu("htrvt_silu_fwd", pre, nullptr, a, n, dtype, false, stream);
}

extern "C" int htrvt_silu_bwd(const void* da, const void* pre, void* dpre, int64_t n, int dtype, void* stream) {
  return silu("htrvt_silu_bwd", pre, da, dpre, n, dtype, true, stream);
}
