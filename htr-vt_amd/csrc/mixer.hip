// mixer.hip -- the convolutional token mixer of the macaron forks (model_sgm_macaron/model/HTR_VT.py ConvLocalMixer1D)
// between its two Linear layers: GLU -> depthwise Conv1d over the tokens (zero padding per image) -> BatchNorm1d -> SiLU,
// on token rows [B*N][D] as the GEMMs leave them (no transpose, no [B][D][N] copy).
//   htrvt_mixer_fwd_train   u [B*N][2D] -> c [B*N][D] = dwconv(glu(u)), + per-workgroup partial rows (sum c, sum c^2)
//                           for htrvt_bn_finalize
//   htrvt_mixer_bn_silu     s = silu(c * scale + shift), the second pass of the train forward
//   htrvt_mixer_fwd_eval    one launch: s = silu(dwconv(glu(u)) * scale + shift); c is written too where a backward follows
//   htrvt_mixer_bwd_reduce  dz = ds * silu'(z), z = c * scale + shift: partial rows (sum dz, sum dz * xhat) for
//                           htrvt_bn_bwd_finalize
//   htrvt_mixer_bwd         dc = cA * dz + cB * c + cC on the fly, dg = dc convolved with the flipped taps, the GLU
//                           recomputed from u -> du [B*N][2D]; partial rows of d weight [D][k] (and d bias)
// Work split: a thread owns one 16-byte channel vector and walks a run of `tl` tokens of one image with a k-row register
// window, so a row of the input is read once by its owner and k - 1 more times only at the ends of a run (from the L2).
// A workgroup is cw channel vectors x 256 / cw runs; its partial sums are combined through LDS in a fixed order and
// written as one row: no float atomics, every result is bitwise reproducible.
#include "rowvec.h"

using namespace htrvt;

namespace {

constexpr int NT = ROWVEC_NT;
constexpr int MAXK = 15;

// the split of a shape into runs: tl tokens per run, cw = 1 << lcw channel vectors per workgroup
struct Split {
  int tl, lcw, gx, gy;
};

inline bool make_split(int B, int N, int D, int dtype, Split* s) {
  const int dv = D / (dtype == HTRVT_BF16 ? 8 : 4);
  int lcw = 0;
  while ((1 << lcw) < dv && lcw < 5) ++lcw;
  int tl = 16;   // shorter runs until the launch has three waves per SIMD (256 CUs x 4 SIMDs x 3 x 64 threads)
  while (tl > 4 && (long long)B * ((N + tl - 1) / tl) * dv < 196608) tl >>= 1;
  const int rpb = NT >> lcw;
  long long gy = ((long long)B * ((N + tl - 1) / tl) + rpb - 1) / rpb;
  while (gy > 65535 && tl < N) {
    tl <<= 1;
    gy = ((long long)B * ((N + tl - 1) / tl) + rpb - 1) / rpb;
  }
  if (gy > 65535) return false;
  s->tl = tl;
  s->lcw = lcw;
  s->gx = (dv + (1 << lcw) - 1) >> lcw;
  s->gy = (int)gy;
  return true;
}

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + __expf(-x)); }

// one thread's place: channel vector cv, image b, tokens [t0, t1)
struct Place {
  int cv, cl, rl, b, t0, t1;
  bool active;
};
__device__ __forceinline__ Place my_place(int B, int N, int dv, int tl, int lcw) {
  Place p;
  p.cl = threadIdx.x & ((1 << lcw) - 1);
  p.rl = threadIdx.x >> lcw;
  p.cv = (blockIdx.x << lcw) + p.cl;
  const int cpi = (N + tl - 1) / tl;
  const long long run = (long long)blockIdx.y * (NT >> lcw) + p.rl;
  p.active = p.cv < dv && run < (long long)B * cpi;
  p.b = p.active ? (int)(run / cpi) : 0;
  p.t0 = p.active ? (int)(run % cpi) * tl : 0;
  p.t1 = p.active ? min(N, p.t0 + tl) : 0;
  return p;
}

// ------------------------------------------------------------------ forward
// the two halves of u's row of token t of the image whose first row is `base`, as loaded; `in`: t is inside 0 .. N-1
template <typename T>
struct URow {
  Vec16<T> a, b;
  bool in;
};
template <typename T>
__device__ __forceinline__ URow<T> ld_urow(const T* __restrict__ u, long long base, int t, int N, int D, int c0) {
  URow<T> r;
  r.in = t >= 0 && t < N;
  if (r.in) {
    const long long o = (base + t) * 2 * D + c0;
    r.a = ld_vec(u, o);
    r.b = ld_vec(u, o + D);
  }
  return r;
}
// g = value half * sigmoid(gate half); zero outside the image
template <typename T>
__device__ __forceinline__ void glu_row(const URow<T>& r, float (&g)[Vec16<T>::N]) {
#pragma unroll
  for (int e = 0; e < Vec16<T>::N; ++e) g[e] = r.in ? r.a.get(e) * sigmoid_f(r.b.get(e)) : 0.f;
}

// TRAIN: writes c and the partial row (sum c, sum c^2) of the workgroup.  Otherwise: s = silu(c * scale + shift)
// (scale == NULL: 1, shift == NULL: 0), and c where cout != NULL.  The statistics and z are taken from c as it is stored
// (rounded to T), which is what the second pass and the backward read.
template <typename T, int K, bool TRAIN>
__global__ __launch_bounds__(NT) void mixer_fwd_kernel(const T* __restrict__ u, const float* __restrict__ w,
                                                       const float* __restrict__ scale, const float* __restrict__ shift,
                                                       T* __restrict__ cout, T* __restrict__ sout,
                                                       float* __restrict__ partial, int B, int N, int D, int tl, int lcw) {
  constexpr int CH = Vec16<T>::N, P = K / 2;
  __shared__ float red[NT * CH];
  const Place p = my_place(B, N, D / CH, tl, lcw);
  const int c0 = p.cv * CH;
  float s1[CH], s2[CH];
#pragma unroll
  for (int e = 0; e < CH; ++e) s1[e] = s2[e] = 0.f;
  if (p.active) {
    float wt[K][CH], sc[CH], sh[CH], win[K][CH];
#pragma unroll
    for (int e = 0; e < CH; ++e)
#pragma unroll
      for (int j = 0; j < K; ++j) wt[j][e] = w[(long long)(c0 + e) * K + j];
    ld_coef<CH>(TRAIN ? nullptr : scale, c0, 1.f, sc);
    ld_coef<CH>(TRAIN ? nullptr : shift, c0, 0.f, sh);
    const long long base = (long long)p.b * N;
#pragma unroll
    for (int i = 1; i < K; ++i) glu_row(ld_urow(u, base, p.t0 - P + i - 1, N, D, c0), win[i]);
    URow<T> nxt = ld_urow(u, base, p.t0 + P, N, D, c0);
    for (int n = p.t0; n < p.t1; ++n) {
      const URow<T> cur = nxt;
      if (n + 1 < p.t1) nxt = ld_urow(u, base, n + 1 + P, N, D, c0);     // the next row is in flight during this one
#pragma unroll
      for (int i = 0; i + 1 < K; ++i)
#pragma unroll
        for (int e = 0; e < CH; ++e) win[i][e] = win[i + 1][e];
      glu_row(cur, win[K - 1]);
      Vec16<T> cv, sv;
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < K; ++j) a = fmaf(wt[j][e], win[j][e], a);
        const float cr = to_f32(from_f32<T>(a));
        cv.set(e, cr);
        if (TRAIN) {
          s1[e] += cr;
          s2[e] = fmaf(cr, cr, s2[e]);
        } else {
          const float z = fmaf(cr, sc[e], sh[e]);
          sv.set(e, z * sigmoid_f(z));
        }
      }
      const long long o = (base + n) * D + c0;
      if (cout) st_vec(cout, o, cv);
      if (!TRAIN) st_vec(sout, o, sv);
    }
  }
  if (TRAIN) {
    run_sum<CH>(s1, red, p.cl, p.rl, lcw);
    run_sum<CH>(s2, red, p.cl, p.rl, lcw);
    if (p.rl == 0 && p.cv < D / CH) {
      float* row = partial + (long long)blockIdx.y * 2 * D + c0;
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        row[e] = s1[e];
        row[D + e] = s2[e];
      }
    }
  }
}

// s = silu(c * scale + shift); a thread owns a channel vector and takes the rows blockIdx.y * rpb + rl, + gridDim.y * rpb, ...
template <typename T>
__global__ __launch_bounds__(NT) void mixer_bn_silu_kernel(const T* __restrict__ c, const float* __restrict__ scale,
                                                           const float* __restrict__ shift, T* __restrict__ s,
                                                           long long rows, int D, int lcw) {
  constexpr int CH = Vec16<T>::N, U = 4;
  const int cl = threadIdx.x & ((1 << lcw) - 1), rl = threadIdx.x >> lcw;
  const int cv = (blockIdx.x << lcw) + cl, c0 = cv * CH;
  if (cv >= D / CH) return;
  float sc[CH], sh[CH];
  ld_coef<CH>(scale, c0, 1.f, sc);
  ld_coef<CH>(shift, c0, 0.f, sh);
  const long long step = (long long)gridDim.y * (NT >> lcw);
  for (long long r = (long long)blockIdx.y * (NT >> lcw) + rl; r < rows; r += U * step) {
    Vec16<T> x[U];
#pragma unroll
    for (int q = 0; q < U; ++q)
      if (r + q * step < rows) x[q] = ld_vec(c, (r + q * step) * D + c0);
#pragma unroll
    for (int q = 0; q < U; ++q) {
      if (r + q * step >= rows) break;
      Vec16<T> y;
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        const float z = fmaf(x[q].get(e), sc[e], sh[e]);
        y.set(e, z * sigmoid_f(z));
      }
      st_vec(s, (r + q * step) * D + c0, y);
    }
  }
}

// ------------------------------------------------------------------ backward
// dz = ds * silu'(z), z = c * sc + sh
__device__ __forceinline__ float silu_bwd(float ds, float z) {
  const float sg = sigmoid_f(z);
  return ds * sg * fmaf(z, 1.f - sg, 1.f);
}

// partial[blockIdx.y] = (sum dz, sum dz * (c - mean) * rstd) over the rows blockIdx.y * rpb + rl, + gridDim.y * rpb, ...
// mean == NULL: the second sum is zero
template <typename T>
__global__ __launch_bounds__(NT) void mixer_bwd_reduce_kernel(const T* __restrict__ ds, const T* __restrict__ c,
                                                              const float* __restrict__ scale, const float* __restrict__ shift,
                                                              const float* __restrict__ mean, const float* __restrict__ rstd,
                                                              float* __restrict__ partial, long long rows, int D, int lcw) {
  constexpr int CH = Vec16<T>::N;
  __shared__ float red[NT * CH];
  const int cl = threadIdx.x & ((1 << lcw) - 1), rl = threadIdx.x >> lcw, rpb = NT >> lcw;
  const int cv = (blockIdx.x << lcw) + cl, c0 = cv * CH;
  const bool active = cv < D / CH;
  float s1[CH], s2[CH];
#pragma unroll
  for (int e = 0; e < CH; ++e) s1[e] = s2[e] = 0.f;
  if (active) {
    constexpr int U = 4;      // rows in flight per thread
    float sc[CH], sh[CH], mu[CH], rs[CH];
    ld_coef<CH>(scale, c0, 1.f, sc);
    ld_coef<CH>(shift, c0, 0.f, sh);
    ld_coef<CH>(mean, c0, 0.f, mu);
    ld_coef<CH>(mean ? rstd : nullptr, c0, 0.f, rs);
    const long long step = (long long)gridDim.y * rpb;
    for (long long r = (long long)blockIdx.y * rpb + rl; r < rows; r += U * step) {
      Vec16<T> dv[U], xv[U];
#pragma unroll
      for (int q = 0; q < U; ++q)
        if (r + q * step < rows) {
          dv[q] = ld_vec(ds, (r + q * step) * D + c0);
          xv[q] = ld_vec(c, (r + q * step) * D + c0);
        }
#pragma unroll
      for (int q = 0; q < U; ++q) {      // rows in increasing order: the sums do not depend on U
        if (r + q * step >= rows) break;
#pragma unroll
        for (int e = 0; e < CH; ++e) {
          const float x = xv[q].get(e);
          const float dz = silu_bwd(dv[q].get(e), fmaf(x, sc[e], sh[e]));
          s1[e] += dz;
          s2[e] = fmaf(dz, (x - mu[e]) * rs[e], s2[e]);
        }
      }
    }
  }
  run_sum<CH>(s1, red, cl, rl, lcw);
  run_sum<CH>(s2, red, cl, rl, lcw);
  if (rl == 0 && active) {
    float* row = partial + (long long)blockIdx.y * 2 * D + c0;
#pragma unroll
    for (int e = 0; e < CH; ++e) {
      row[e] = s1[e];
      row[D + e] = s2[e];
    }
  }
}

// ds and c of token t as loaded; dc = cA * dz + cB * c + cC of it (zero outside 0 .. N-1)
template <typename T>
struct GRow {
  Vec16<T> ds, c;
  bool in;
};
template <typename T>
__device__ __forceinline__ GRow<T> ld_grow(const T* __restrict__ ds, const T* __restrict__ c, long long base, int t, int N, int D,
                                           int c0) {
  GRow<T> r;
  r.in = t >= 0 && t < N;
  if (r.in) {
    const long long o = (base + t) * D + c0;
    r.ds = ld_vec(ds, o);
    r.c = ld_vec(c, o);
  }
  return r;
}
template <typename T>
__device__ __forceinline__ void dc_row(const GRow<T>& r, const float (&sc)[Vec16<T>::N], const float (&sh)[Vec16<T>::N],
                                       const float (&cA)[Vec16<T>::N], const float (&cB)[Vec16<T>::N],
                                       const float (&cC)[Vec16<T>::N], float (&out)[Vec16<T>::N]) {
#pragma unroll
  for (int e = 0; e < Vec16<T>::N; ++e) {
    const float x = r.in ? r.c.get(e) : 0.f;
    const float dz = silu_bwd(r.in ? r.ds.get(e) : 0.f, fmaf(x, sc[e], sh[e]));
    out[e] = r.in ? fmaf(cA[e], dz, fmaf(cB[e], x, cC[e])) : 0.f;
  }
}

// du and the workgroup's partial row of d weight (pw [gridDim.y][D * K], element d * K + j) and, where pb != NULL, of
// d bias (pb [gridDim.y][D]).  With win[i] = dc(n + i - P):  dg(n) = sum_i w[K-1-i] * win[i]  and
// d w[j] += g(n) * dc(n + P - j) = g(n) * win[K-1-j]
template <typename T, int K>
__global__ __launch_bounds__(NT) void mixer_bwd_kernel(const T* __restrict__ u, const T* __restrict__ c, const T* __restrict__ ds,
                                                       const float* __restrict__ w, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, const float* __restrict__ coef,
                                                       T* __restrict__ du, float* __restrict__ pw, float* __restrict__ pb,
                                                       int B, int N, int D, int tl, int lcw) {
  constexpr int CH = Vec16<T>::N, P = K / 2;
  __shared__ float red[NT * CH];
  const Place p = my_place(B, N, D / CH, tl, lcw);
  const int c0 = p.cv * CH;
  float dw[K][CH], db[CH];
#pragma unroll
  for (int e = 0; e < CH; ++e) {
    db[e] = 0.f;
#pragma unroll
    for (int j = 0; j < K; ++j) dw[j][e] = 0.f;
  }
  if (p.active) {
    float wt[K][CH], sc[CH], sh[CH], cA[CH], cB[CH], cC[CH], win[K][CH];
#pragma unroll
    for (int e = 0; e < CH; ++e)
#pragma unroll
      for (int j = 0; j < K; ++j) wt[j][e] = w[(long long)(c0 + e) * K + j];
    ld_coef<CH>(scale, c0, 1.f, sc);
    ld_coef<CH>(shift, c0, 0.f, sh);
    ld_coef<CH>(coef, c0, 1.f, cA);
    ld_coef<CH>(coef ? coef + D : nullptr, c0, 0.f, cB);
    ld_coef<CH>(coef ? coef + 2 * D : nullptr, c0, 0.f, cC);
    const long long base = (long long)p.b * N;
#pragma unroll
    for (int i = 1; i < K; ++i) dc_row(ld_grow(ds, c, base, p.t0 - P + i - 1, N, D, c0), sc, sh, cA, cB, cC, win[i]);
    // (no row is loaded ahead here, unlike the forward: the four more vectors take the bfloat16 k = 7 kernel past 256
    // registers, one wave per SIMD instead of two, and the launch from 62 to 86 us at B = N = 128, D = 768)
    for (int n = p.t0; n < p.t1; ++n) {
      const GRow<T> gcur = ld_grow(ds, c, base, n + P, N, D, c0);
      const URow<T> ucur = ld_urow(u, base, n, N, D, c0);
#pragma unroll
      for (int i = 0; i + 1 < K; ++i)
#pragma unroll
        for (int e = 0; e < CH; ++e) win[i][e] = win[i + 1][e];
      dc_row(gcur, sc, sh, cA, cB, cC, win[K - 1]);
      const long long o = (base + n) * 2 * D + c0;
      const Vec16<T>&a = ucur.a, &bb = ucur.b;
      Vec16<T> da, dbv;
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        float dg = 0.f;
#pragma unroll
        for (int i = 0; i < K; ++i) dg = fmaf(wt[K - 1 - i][e], win[i][e], dg);
        const float av = a.get(e), sg = sigmoid_f(bb.get(e));
        const float g = av * sg;
#pragma unroll
        for (int j = 0; j < K; ++j) dw[j][e] = fmaf(g, win[K - 1 - j][e], dw[j][e]);
        db[e] += win[P][e];
        da.set(e, dg * sg);
        dbv.set(e, dg * g * (1.f - sg));
      }
      st_vec(du, o, da);
      st_vec(du, o + D, dbv);
    }
  }
  const bool writer = p.rl == 0 && p.cv < D / CH;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    run_sum<CH>(dw[j], red, p.cl, p.rl, lcw);
    if (writer) {
      float* row = pw + (long long)blockIdx.y * D * K;
#pragma unroll
      for (int e = 0; e < CH; ++e) row[(long long)(c0 + e) * K + j] = dw[j][e];
    }
  }
  if (pb) {
    run_sum<CH>(db, red, p.cl, p.rl, lcw);
    if (writer) {
#pragma unroll
      for (int e = 0; e < CH; ++e) pb[(long long)blockIdx.y * D + c0 + e] = db[e];
    }
  }
}

// ------------------------------------------------------------------ host side
int check_shape(const char* what, int B, int N, int D, int k, int dtype) {
  HTRVT_REQUIRE(dtype == HTRVT_F32 || dtype == HTRVT_BF16, "%s: dtype %d", what, dtype);
  HTRVT_REQUIRE(B >= 1 && N >= 1 && D >= 8, "%s: B=%d N=%d D=%d", what, B, N, D);
  HTRVT_REQUIRE(D % 8 == 0, "%s: D=%d is not a multiple of 8", what, D);
  HTRVT_REQUIRE(k >= 1 && k <= MAXK && (k & 1), "%s: kernel size %d (odd, 1 ... %d)", what, k, MAXK);
  HTRVT_REQUIRE((long long)B * N < (1ll << 31), "%s: too many rows", what);
  return 0;
}

#define MIXER_BY_K(k, LAUNCH)   \
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

template <typename T, bool TRAIN>
void launch_fwd(const Split& sp, hipStream_t st, int k, const void* u, const float* w, const float* scale, const float* shift,
                void* c, void* s, float* partial, int B, int N, int D) {
  const dim3 grid(sp.gx, sp.gy);
#define LAUNCH(KK)                                                                                                          \
  hipLaunchKernelGGL((mixer_fwd_kernel<T, KK, TRAIN>), grid, dim3(NT), 0, st, (const T*)u, w, scale, shift, (T*)c, (T*)s, \
                     partial, B, N, D, sp.tl, sp.lcw)
  MIXER_BY_K(k, LAUNCH)
#undef LAUNCH
}

template <typename T>
void launch_bwd(const Split& sp, hipStream_t st, int k, const void* u, const void* c, const void* ds, const float* w,
                const float* scale, const float* shift, const float* coef, void* du, float* pw, float* pb, int B, int N, int D) {
  const dim3 grid(sp.gx, sp.gy);
#define LAUNCH(KK)                                                                                                        \
  hipLaunchKernelGGL((mixer_bwd_kernel<T, KK>), grid, dim3(NT), 0, st, (const T*)u, (const T*)c, (const T*)ds, w, scale, \
                     shift, coef, (T*)du, pw, pb, B, N, D, sp.tl, sp.lcw)
  MIXER_BY_K(k, LAUNCH)
#undef LAUNCH
}

int reduce_rows(long long rows, int D, int dtype) {
  const int dv = D / (dtype == HTRVT_BF16 ? 8 : 4);
  int lcw = 0;
  while ((1 << lcw) < dv && lcw < 5) ++lcw;
  const int rpb = NT >> lcw;
  const long long n = (rows + rpb - 1) / rpb;
  return (int)(n < 1 ? 1 : (n > 128 ? 128 : n));
}

}  // namespace

extern "C" int htrvt_mixer_rows(int B, int N, int D, int dtype) {
  if (check_shape("htrvt_mixer_rows", B, N, D, 1, dtype)) return -1;
  Split sp;
  HTRVT_REQUIRE(make_split(B, N, D, dtype, &sp), "htrvt_mixer_rows: B=%d N=%d does not fit one launch", B, N);
  return sp.gy;
}

extern "C" int64_t htrvt_mixer_fwd_workspace_floats(int B, int N, int D, int dtype) {
  const int rows = htrvt_mixer_rows(B, N, D, dtype);
  return rows < 0 ? -1 : ((int64_t)rows + 64) * 2 * D;     // + the 64 scratch rows htrvt_bn_finalize asks for
}

extern "C" int64_t htrvt_mixer_bwd_workspace_floats(int B, int N, int D, int k, int dtype) {
  const int rows = htrvt_mixer_rows(B, N, D, dtype);
  return rows < 0 ? -1 : (int64_t)rows * D * (k + 1);
}

extern "C" int htrvt_mixer_reduce_rows(int64_t rows, int D, int dtype) {
  HTRVT_REQUIRE(rows >= 1 && D >= 8 && D % 8 == 0, "htrvt_mixer_reduce_rows: rows=%lld D=%d", (long long)rows, D);
  return reduce_rows(rows, D, dtype);
}

extern "C" int htrvt_mixer_fwd_train(const void* u, const float* w, void* c, float* partial, int B, int N, int D, int k,
                                     int dtype, void* stream) {
  if (check_shape("htrvt_mixer_fwd_train", B, N, D, k, dtype)) return -1;
  HTRVT_REQUIRE((long long)B * N >= 2, "htrvt_mixer_fwd_train: batch statistics need B * N >= 2 values per channel");
  HTRVT_REQUIRE(u && w && c && partial, "htrvt_mixer_fwd_train: null buffer");
  HTRVT_REQUIRE(!misaligned16(u, c), "htrvt_mixer_fwd_train: u / c not 16-byte aligned");
  Split sp;
  HTRVT_REQUIRE(make_split(B, N, D, dtype, &sp), "htrvt_mixer_fwd_train: B=%d N=%d does not fit one launch", B, N);
  if (dtype == HTRVT_BF16)
    launch_fwd<bf16_t, true>(sp, (hipStream_t)stream, k, u, w, nullptr, nullptr, c, nullptr, partial, B, N, D);
  else
    launch_fwd<float, true>(sp, (hipStream_t)stream, k, u, w, nullptr, nullptr, c, nullptr, partial, B, N, D);
  return check_launch("mixer_fwd_train");
}

extern "C" int htrvt_mixer_bn_silu(const void* c, const float* scale, const float* shift, void* s, int64_t rows, int D,
                                   int dtype, void* stream) {
  HTRVT_REQUIRE(dtype == HTRVT_F32 || dtype == HTRVT_BF16, "htrvt_mixer_bn_silu: dtype %d", dtype);
  HTRVT_REQUIRE(rows >= 0 && D >= 8 && D % 8 == 0, "htrvt_mixer_bn_silu: rows=%lld, D=%d (a multiple of 8)", (long long)rows, D);
  if (rows == 0) return 0;
  HTRVT_REQUIRE(c && s, "htrvt_mixer_bn_silu: null buffer");
  HTRVT_REQUIRE(!misaligned16(c, s), "htrvt_mixer_bn_silu: c / s not 16-byte aligned");
  const int dv = D / (dtype == HTRVT_BF16 ? 8 : 4);
  int lcw = 0;
  while ((1 << lcw) < dv && lcw < 5) ++lcw;
  const long long gy = (rows + 4 * (NT >> lcw) - 1) / (4 * (NT >> lcw));      // four rows per thread
  const dim3 grid((dv + (1 << lcw) - 1) >> lcw, (unsigned)(gy > 16384 ? 16384 : gy));
  if (dtype == HTRVT_BF16)
    hipLaunchKernelGGL(mixer_bn_silu_kernel<bf16_t>, grid, dim3(NT), 0, (hipStream_t)stream, (const bf16_t*)c, scale, shift,
                       (bf16_t*)s, (long long)rows, D, lcw);
  else
    hipLaunchKernelGGL(mixer_bn_silu_kernel<float>, grid, dim3(NT), 0, (hipStream_t)stream, (const float*)c, scale, shift,
                       (float*)s, (long long)rows, D, lcw);
  return check_launch("mixer_bn_silu");
}

extern "C" int htrvt_mixer_fwd_eval(const void* u, const float* w, const float* scale, const float* shift, void* c, void* s,
                                    int B, int N, int D, int k, int dtype, void* stream) {
  if (check_shape("htrvt_mixer_fwd_eval", B, N, D, k, dtype)) return -1;
  HTRVT_REQUIRE(u && w && s, "htrvt_mixer_fwd_eval: null buffer");
  HTRVT_REQUIRE(!misaligned16(u, c, s), "htrvt_mixer_fwd_eval: u / c / s not 16-byte aligned");
  Split sp;
  HTRVT_REQUIRE(make_split(B, N, D, dtype, &sp), "htrvt_mixer_fwd_eval: B=%d N=%d does not fit one launch", B, N);
  if (dtype == HTRVT_BF16)
    launch_fwd<bf16_t, false>(sp, (hipStream_t)stream, k, u, w, scale, shift, c, s, nullptr, B, N, D);
  else
    launch_fwd<float, false>(sp, (hipStream_t)stream, k, u, w, scale, shift, c, s, nullptr, B, N, D);
  return check_launch("mixer_fwd_eval");
}

extern "C" int htrvt_mixer_bwd_reduce(const void* ds, const void* c, const float* scale, const float* shift, const float* mean,
                                      const float* rstd, float* partial, int64_t rows, int D, int dtype, void* stream) {
  HTRVT_REQUIRE(dtype == HTRVT_F32 || dtype == HTRVT_BF16, "htrvt_mixer_bwd_reduce: dtype %d", dtype);
  HTRVT_REQUIRE(rows >= 1 && D >= 8 && D % 8 == 0, "htrvt_mixer_bwd_reduce: rows=%lld, D=%d (a multiple of 8)", (long long)rows, D);
  HTRVT_REQUIRE(ds && c && partial && (!mean || rstd), "htrvt_mixer_bwd_reduce: null buffer");
  HTRVT_REQUIRE(!misaligned16(ds, c), "htrvt_mixer_bwd_reduce: ds / c not 16-byte aligned");
  const int dv = D / (dtype == HTRVT_BF16 ? 8 : 4);
  int lcw = 0;
  while ((1 << lcw) < dv && lcw < 5) ++lcw;
  const dim3 grid((dv + (1 << lcw) - 1) >> lcw, reduce_rows(rows, D, dtype));
  if (dtype == HTRVT_BF16)
    hipLaunchKernelGGL(mixer_bwd_reduce_kernel<bf16_t>, grid, dim3(NT), 0, (hipStream_t)stream, (const bf16_t*)ds,
                       (const bf16_t*)c, scale, shift, mean, rstd, partial, (long long)rows, D, lcw);
  else
    hipLaunchKernelGGL(mixer_bwd_reduce_kernel<float>, grid, dim3(NT), 0, (hipStream_t)stream, (const float*)ds,
                       (const float*)c, scale, shift, mean, rstd, partial, (long long)rows, D, lcw);
  return check_launch("mixer_bwd_reduce");
}

extern "C" int htrvt_mixer_bwd(const void* u, const void* c, const void* ds, const float* w, const float* scale,
                               const float* shift, const float* coef, void* du, float* dw_partial, float* db_partial, int B,
                               int N, int D, int k, int dtype, void* stream) {
  if (check_shape("htrvt_mixer_bwd", B, N, D, k, dtype)) return -1;
  HTRVT_REQUIRE(u && c && ds && w && du && dw_partial, "htrvt_mixer_bwd: null buffer");
  HTRVT_REQUIRE(!misaligned16(u, c, ds, du), "htrvt_mixer_bwd: u / c / ds / du not 16-byte aligned");
  Split sp;
  HTRVT_REQUIRE(make_split(B, N, D, dtype, &sp), "htrvt_mixer_bwd: B=%d N=%d does not fit one launch", B, N);
  if (dtype == HTRVT_BF16)
    launch_bwd<bf16_t>(sp, (hipStream_t)stream, k, u, c, ds, w, scale, shift, coef, du, dw_partial, db_partial, B, N, D);
  else
    launch_bwd<float>(sp, (hipStream_t)stream, k, u, c, ds, w, scale, shift, coef, du, dw_partial, db_partial, B, N, D);
  return check_launch("mixer_bwd");
}
