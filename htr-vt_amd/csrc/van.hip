// van.hip -- the operators of the VAN forks' height reducer and horizontal mixer (model_sgm_mms_attach_van/model/HTR_VT.py:
// LargeKernelAttention, VANBlock, VANHeightReducer, HorizontalMixer) that are not GEMMs or BatchNorm passes, on NHWC
// activations [B][H][W][C]:
//   htrvt_van_dw_fwd         depthwise 2-D convolution, kh x kw taps with dilation, zero padding per image
//   htrvt_van_dw_bwd_input   its input gradient: the same kernel over the flipped taps (+ an optional tensor added last)
//   htrvt_van_dw_bwd_weight  its weight gradient as partial rows [R][C * kh * kw] for htrvt_colsum
//   htrvt_van_moments        partial rows (sum x, sum x^2) per channel for htrvt_bn_finalize
//   htrvt_van_gate_fwd/_bwd  the LKA gate  g = a * (p * scale + shift)
//   htrvt_van_bn_res_gelu_fwd/_bwd   y = gelu(res + x * scale + shift) of the horizontal mixer
//   htrvt_van_hpool_fwd/_bwd the mean over H
// Work split of the convolutions: a thread owns one 16-byte channel vector and a run of TL output pixels of ONE image row
// that lie `dil` apart, w0 + q * dil; the inputs of one kernel row for that run are the TL + kw - 1 pixels w0 + (s - kw/2)
// * dil, loaded once into registers and used by up to kw outputs each -- the reuse does not depend on the dilation.  A
// workgroup is cw channel vectors x 256 / cw runs of one image row (b, h), so which kernel rows fall outside the image is
// the same for all of its threads: a dead kernel row is skipped by the (uniform) row loop, costing no loads and no FMAs,
// and its taps are not staged either.  The taps of the live rows sit in LDS as [tap][channel], read as 16-byte vectors.
// Reductions are per-workgroup partial rows combined through LDS in a fixed order: no float atomics.
#include "gemm_common.h"
#include "rowvec.h"

using namespace htrvt;

namespace {

constexpr int NT = ROWVEC_NT;
constexpr int TL = 4;            // output pixels per run
constexpr int MAXKH = 7, MAXKW = 9, MAXDIL = 3;
constexpr int WLDS = 8192;       // floats of LDS for the staged taps: (CH << lcw) channels x the live taps

struct Geo {
  int lcw, rc, tiles, gx;        // cw = 1 << lcw; rc runs per residue class of w mod dil; tiles of 256 >> lcw runs per row
};

inline Geo make_geo(int W, int C, int kh, int kw, int dil, int dtype) {
  const int ch = dtype == HTRVT_BF16 ? 8 : 4, dv = C / ch;
  Geo g;
  g.lcw = 0;
  while ((1 << g.lcw) < dv && g.lcw < 5) ++g.lcw;
  while (g.lcw > 0 && (ch << g.lcw) * kh * kw > WLDS) --g.lcw;
  g.rc = ((W + dil - 1) / dil + TL - 1) / TL;
  const int rpb = NT >> g.lcw;
  g.tiles = (dil * g.rc + rpb - 1) / rpb;
  g.gx = (dv + (1 << g.lcw) - 1) >> g.lcw;
  return g;
}

// kernel rows i0 .. i1 - 1 of output row h read rows inside the image: 0 <= h + (i - kh/2) * dil < H
__device__ __forceinline__ void live_rows(int h, int H, int kh, int dil, int& i0, int& i1) {
  i0 = max(0, kh / 2 - h / dil);
  i1 = min(kh, kh / 2 + (H - 1 - h) / dil + 1);
}

// one thread's place in a row of W pixels: channel vector cv, first output pixel w0 (the others are w0 + q * dil)
struct Place {
  int cl, rl, cv, w0;
  bool active;
};
__device__ __forceinline__ Place my_place(int tile, int dv, int dil, int rc, int lcw) {
  Place p;
  p.cl = threadIdx.x & ((1 << lcw) - 1);
  p.rl = threadIdx.x >> lcw;
  p.cv = (blockIdx.x << lcw) + p.cl;
  const int run = tile * (NT >> lcw) + p.rl;
  p.active = p.cv < dv && run < dil * rc;
  p.w0 = p.active ? run / rc + (run % rc) * TL * dil : 0;
  return p;
}

// the TL + KW - 1 input vectors of a run in the row that starts at element `row` (channel offset included); zeros outside
// 0 .. W-1
template <typename T, int KW>
__device__ __forceinline__ void ld_window(const T* __restrict__ x, long long row, int w0, int dil, int W, int C,
                                          Vec16<T> (&xs)[TL + KW - 1]) {
#pragma unroll
  for (int s = 0; s < TL + KW - 1; ++s) {
    const int ww = w0 + (s - KW / 2) * dil;
    if (ww >= 0 && ww < W) {
      xs[s] = ld_vec(x, row + (long long)ww * C);
    } else {
      xs[s].raw.x = xs[s].raw.y = xs[s].raw.z = xs[s].raw.w = 0;
    }
  }
}

// ------------------------------------------------------------------ depthwise convolution, forward and input gradient
// y[b][h][w][c] = sum_ij wt[c][i * KW + j] * x[b][h + (i - kh/2) dil][w + (j - KW/2) dil][c]  (+ add).  flip: the taps are
// read as wt[c][(kh-1-i) * KW + (KW-1-j)], which makes the same sum the input gradient of the convolution.
// grid (channel blocks, tiles of runs, B * H)
template <typename T, int KW>
__global__ __launch_bounds__(NT) void dw_conv_kernel(const T* __restrict__ x, const float* __restrict__ wt,
                                                     const T* __restrict__ add, T* __restrict__ y, int H, int W, int C, int kh,
                                                     int dil, int flip, int lcw, int rc) {
  constexpr int CH = Vec16<T>::N;
  __shared__ __attribute__((aligned(16))) float wl[WLDS];
  const int bh = blockIdx.z, h = bh % H;
  int i0, i1;
  live_rows(h, H, kh, dil, i0, i1);
  const int nch = CH << lcw, cb = blockIdx.x * nch, ntap = (i1 - i0) * KW;
  for (int t = threadIdx.x; t < nch * ntap; t += NT) {
    const int ch = t / ntap, r = t % ntap, i = i0 + r / KW, j = r % KW;
    const int src = flip ? (kh - 1 - i) * KW + (KW - 1 - j) : i * KW + j;
    wl[r * nch + ch] = cb + ch < C ? wt[(long long)(cb + ch) * kh * KW + src] : 0.f;
  }
  __syncthreads();
  const Place p = my_place(blockIdx.y, C / CH, dil, rc, lcw);
  if (!p.active) return;
  const int c0 = p.cv * CH;
  float acc[TL][CH];
#pragma unroll
  for (int q = 0; q < TL; ++q)
#pragma unroll
    for (int e = 0; e < CH; ++e) acc[q][e] = 0.f;
  for (int il = 0; il < i1 - i0; ++il) {
    const int hh = h + (i0 + il - kh / 2) * dil;
    Vec16<T> xs[TL + KW - 1];
    ld_window<T, KW>(x, ((long long)(bh - h + hh) * W) * C + c0, p.w0, dil, W, C, xs);
#pragma unroll
    for (int j = 0; j < KW; ++j) {
      float wv[CH];
      ld_coef<CH>(wl, (il * KW + j) * nch + p.cl * CH, 0.f, wv);
#pragma unroll
      for (int q = 0; q < TL; ++q)
#pragma unroll
        for (int e = 0; e < CH; ++e) acc[q][e] = fmaf(wv[e], xs[q + j].get(e), acc[q][e]);
    }
  }
  const long long orow = ((long long)bh * W) * C + c0;
#pragma unroll
  for (int q = 0; q < TL; ++q) {
    const int w = p.w0 + q * dil;
    if (w >= W) break;
    Vec16<T> o, a;
    if (add) a = ld_vec(add, orow + (long long)w * C);
#pragma unroll
    for (int e = 0; e < CH; ++e) o.set(e, add ? acc[q][e] + a.get(e) : acc[q][e]);
    st_vec(y, orow + (long long)w * C, o);
  }
}

// ------------------------------------------------------------------ depthwise convolution, weight gradient
// d wt[c][i * KW + j] = sum_bhw dy[b][h][w][c] * x[b][h + (i - kh/2) dil][w + (j - KW/2) dil][c].  grid (channel blocks,
// nchunk, H): the workgroup (chunk, h) takes the items (image, tile of runs) chunk, chunk + nchunk, ... of output row h,
// one kernel row at a time, and writes row h * nchunk + chunk of the partial sums [H * nchunk][C * kh * KW]; the taps of
// a kernel row that is dead for this h are written as zeros.
template <typename T, int KW>
__global__ __launch_bounds__(NT) void dw_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                      float* __restrict__ partial, int B, int H, int W, int C, int kh, int dil,
                                                      int lcw, int rc, int tiles) {
  constexpr int CH = Vec16<T>::N;
  __shared__ float red[NT * CH];
  const int h = blockIdx.z, nchunk = gridDim.y, dv = C / CH;
  const int cl = threadIdx.x & ((1 << lcw) - 1), rl = threadIdx.x >> lcw, cv = (blockIdx.x << lcw) + cl, c0 = cv * CH;
  const bool writer = rl == 0 && cv < dv;
  float* prow = partial + ((long long)h * nchunk + blockIdx.y) * C * kh * KW;
  int i0, i1;
  live_rows(h, H, kh, dil, i0, i1);
  for (int i = 0; i < kh; ++i) {
    float dw[KW][CH];
#pragma unroll
    for (int j = 0; j < KW; ++j)
#pragma unroll
      for (int e = 0; e < CH; ++e) dw[j][e] = 0.f;
    const bool live = i >= i0 && i < i1;       // the same for the whole workgroup
    if (live) {
      const int hh = h + (i - kh / 2) * dil;
      for (int item = blockIdx.y; item < B * tiles; item += nchunk) {
        const int b = item / tiles;
        const Place p = my_place(item % tiles, dv, dil, rc, lcw);
        if (!p.active) continue;
        Vec16<T> xs[TL + KW - 1], g[TL];
        ld_window<T, KW>(x, (((long long)b * H + hh) * W) * C + c0, p.w0, dil, W, C, xs);
        const long long grow = (((long long)b * H + h) * W) * C + c0;
#pragma unroll
        for (int q = 0; q < TL; ++q) {
          const int w = p.w0 + q * dil;
          if (w < W) {
            g[q] = ld_vec(dy, grow + (long long)w * C);
          } else {
            g[q].raw.x = g[q].raw.y = g[q].raw.z = g[q].raw.w = 0;
          }
        }
#pragma unroll
        for (int j = 0; j < KW; ++j)
#pragma unroll
          for (int q = 0; q < TL; ++q)
#pragma unroll
            for (int e = 0; e < CH; ++e) dw[j][e] = fmaf(g[q].get(e), xs[q + j].get(e), dw[j][e]);
      }
#pragma unroll
      for (int j = 0; j < KW; ++j) run_sum<CH>(dw[j], red, cl, rl, lcw);
    }
    if (writer) {
#pragma unroll
      for (int j = 0; j < KW; ++j)
#pragma unroll
        for (int e = 0; e < CH; ++e) prow[(long long)(c0 + e) * kh * KW + i * KW + j] = dw[j][e];
    }
  }
}

// ------------------------------------------------------------------ passes over [rows][C]
// a thread owns a channel vector and takes the rows blockIdx.y * rpb + rl, + gridDim.y * rpb, ...
struct RowWalk {
  int cl, rl, cv, c0;
  long long first, step;
};
template <int CH>
__device__ __forceinline__ RowWalk row_walk(int lcw) {
  RowWalk r;
  r.cl = threadIdx.x & ((1 << lcw) - 1);
  r.rl = threadIdx.x >> lcw;
  r.cv = (blockIdx.x << lcw) + r.cl;
  r.c0 = r.cv * CH;
  r.step = (long long)gridDim.y * (NT >> lcw);
  r.first = (long long)blockIdx.y * (NT >> lcw) + r.rl;
  return r;
}

// partial[blockIdx.y] = (sum x, sum x^2) over the workgroup's rows
template <typename T>
__global__ __launch_bounds__(NT) void moments_kernel(const T* __restrict__ x, float* __restrict__ partial, long long rows, int C,
                                                     int lcw) {
  constexpr int CH = Vec16<T>::N;
  __shared__ float red[NT * CH];
  const RowWalk r = row_walk<CH>(lcw);
  const bool active = r.cv < C / CH;
  float s1[CH], s2[CH];
#pragma unroll
  for (int e = 0; e < CH; ++e) s1[e] = s2[e] = 0.f;
  if (active)
    for (long long n = r.first; n < rows; n += r.step) {
      const Vec16<T> v = ld_vec(x, n * C + r.c0);
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        s1[e] += v.get(e);
        s2[e] = fmaf(v.get(e), v.get(e), s2[e]);
      }
    }
  run_sum<CH>(s1, red, r.cl, r.rl, lcw);
  run_sum<CH>(s2, red, r.cl, r.rl, lcw);
  if (r.rl == 0 && active) {
    float* row = partial + (long long)blockIdx.y * 2 * C + r.c0;
#pragma unroll
    for (int e = 0; e < CH; ++e) {
      row[e] = s1[e];
      row[C + e] = s2[e];
    }
  }
}

enum { EW_GATE_FWD, EW_GATE_BWD, EW_GELU_FWD, EW_GELU_BWD };

// MODE           a    b    c     o1                                        o2
// EW_GATE_FWD    a    p    -     a * (p * scale + shift)
// EW_GATE_BWD    dg   a    p     dg * (p * scale + shift)                  dg * a
// EW_GELU_FWD    x    res  -     gelu(res + x * scale + shift)
// EW_GELU_BWD    dy   x    res   dy * gelu'(res + x * scale + shift)
// scale == NULL: 1, shift == NULL: 0, res == NULL: 0
template <typename T, int MODE>
__global__ __launch_bounds__(NT) void ew_kernel(const T* __restrict__ a, const T* __restrict__ b, const T* __restrict__ c,
                                                const float* __restrict__ scale, const float* __restrict__ shift,
                                                T* __restrict__ o1, T* __restrict__ o2, long long rows, int C, int lcw) {
  constexpr int CH = Vec16<T>::N;
  const RowWalk r = row_walk<CH>(lcw);
  if (r.cv >= C / CH) return;
  float sc[CH], sh[CH];
  ld_coef<CH>(scale, r.c0, 1.f, sc);
  ld_coef<CH>(shift, r.c0, 0.f, sh);
  for (long long n = r.first; n < rows; n += r.step) {
    const long long o = n * C + r.c0;
    const Vec16<T> va = ld_vec(a, o);
    Vec16<T> vb, vc, r1, r2;
    vb.raw.x = vb.raw.y = vb.raw.z = vb.raw.w = 0;
    vc = vb;
    if (b) vb = ld_vec(b, o);
    if (c) vc = ld_vec(c, o);
#pragma unroll
    for (int e = 0; e < CH; ++e) {
      if (MODE == EW_GATE_FWD) {
        r1.set(e, va.get(e) * fmaf(vb.get(e), sc[e], sh[e]));
      } else if (MODE == EW_GATE_BWD) {
        r1.set(e, va.get(e) * fmaf(vc.get(e), sc[e], sh[e]));
        r2.set(e, va.get(e) * vb.get(e));
      } else if (MODE == EW_GELU_FWD) {
        r1.set(e, gelu_erf(vb.get(e) + fmaf(va.get(e), sc[e], sh[e])));
      } else {
        r1.set(e, va.get(e) * gelu_erf_grad(vc.get(e) + fmaf(vb.get(e), sc[e], sh[e])));
      }
    }
    st_vec(o1, o, r1);
    if (MODE == EW_GATE_BWD) st_vec(o2, o, r2);
  }
}

// rows are the B * W pooled pixels.  FWD: y[b][w] = mean_h x[b][h][w]; else dx[b][h][w] = d[b][w] / H
template <typename T, bool FWD>
__global__ __launch_bounds__(NT) void hpool_kernel(const T* __restrict__ in, T* __restrict__ out, long long rows, int H, int W,
                                                   int C, int lcw) {
  constexpr int CH = Vec16<T>::N;
  const RowWalk r = row_walk<CH>(lcw);
  if (r.cv >= C / CH) return;
  const float inv = 1.f / (float)H;
  for (long long n = r.first; n < rows; n += r.step) {
    const long long b = n / W, w = n % W;
    Vec16<T> v;
    if (FWD) {
      float s[CH];
#pragma unroll
      for (int e = 0; e < CH; ++e) s[e] = 0.f;
      for (int h = 0; h < H; ++h) {
        const Vec16<T> xv = ld_vec(in, (((b * H + h) * W) + w) * C + r.c0);
#pragma unroll
        for (int e = 0; e < CH; ++e) s[e] += xv.get(e);
      }
#pragma unroll
      for (int e = 0; e < CH; ++e) v.set(e, s[e] * inv);
      st_vec(out, n * C + r.c0, v);
    } else {
      const Vec16<T> d = ld_vec(in, n * C + r.c0);
#pragma unroll
      for (int e = 0; e < CH; ++e) v.set(e, d.get(e) * inv);
      for (int h = 0; h < H; ++h) st_vec(out, (((b * H + h) * W) + w) * C + r.c0, v);
    }
  }
}

// ------------------------------------------------------------------ host side
int check_conv(const char* what, int B, int H, int W, int C, int kh, int kw, int dil, int dtype) {
  HTRVT_REQUIRE(dtype == HTRVT_F32 || dtype == HTRVT_BF16, "%s: dtype %d", what, dtype);
  HTRVT_REQUIRE(B >= 1 && H >= 1 && W >= 1 && C >= 8, "%s: B=%d H=%d W=%d C=%d", what, B, H, W, C);
  HTRVT_REQUIRE(C % 8 == 0, "%s: C=%d is not a multiple of 8", what, C);
  HTRVT_REQUIRE(kh >= 1 && kh <= MAXKH && (kh & 1), "%s: kernel height %d (odd, 1 ... %d)", what, kh, MAXKH);
  HTRVT_REQUIRE(kw >= 1 && kw <= MAXKW && (kw & 1), "%s: kernel width %d (odd, 1 ... %d)", what, kw, MAXKW);
  HTRVT_REQUIRE(dil >= 1 && dil <= MAXDIL, "%s: dilation %d (1 ... %d)", what, dil, MAXDIL);
  HTRVT_REQUIRE((long long)B * H <= 65535, "%s: B * H = %lld image rows do not fit one launch", what, (long long)B * H);
  HTRVT_REQUIRE((long long)B * H * W < (1ll << 31), "%s: too many pixels", what);
  return 0;
}

int check_rows(const char* what, long long rows, int C, int dtype) {
  HTRVT_REQUIRE(dtype == HTRVT_F32 || dtype == HTRVT_BF16, "%s: dtype %d", what, dtype);
  HTRVT_REQUIRE(rows >= 1 && C >= 8 && C % 8 == 0, "%s: rows=%lld, C=%d (a multiple of 8)", what, rows, C);
  return 0;
}

#define VAN_BY_KW(kw, LAUNCH) \
  switch (kw) {               \
    case 1: LAUNCH(1); break; \
    case 3: LAUNCH(3); break; \
    case 5: LAUNCH(5); break; \
    case 7: LAUNCH(7); break; \
    default: LAUNCH(9); break; \
  }

template <typename T>
void launch_conv(hipStream_t st, const void* x, const float* w, const void* add, void* y, int B, int H, int W, int C, int kh,
                 int kw, int dil, int flip, int dtype) {
  const Geo g = make_geo(W, C, kh, kw, dil, dtype);
  const dim3 grid(g.gx, g.tiles, B * H);
#define LAUNCH(KK)                                                                                                          \
  hipLaunchKernelGGL((dw_conv_kernel<T, KK>), grid, dim3(NT), 0, st, (const T*)x, w, (const T*)add, (T*)y, H, W, C, kh, dil, \
                     flip, g.lcw, g.rc)
  VAN_BY_KW(kw, LAUNCH)
#undef LAUNCH
}

int conv_entry(const char* what, const void* x, const float* w, const void* add, void* y, int B, int H, int W, int C, int kh,
               int kw, int dil, int flip, int dtype, void* stream) {
  if (check_conv(what, B, H, W, C, kh, kw, dil, dtype)) return -1;
  HTRVT_REQUIRE(x && w && y, "%s: null buffer", what);
  HTRVT_REQUIRE(!misaligned16(x, y, add), "%s: a tensor is not 16-byte aligned", what);
  if (dtype == HTRVT_BF16)
    launch_conv<bf16_t>((hipStream_t)stream, x, w, add, y, B, H, W, C, kh, kw, dil, flip, dtype);
  else
    launch_conv<float>((hipStream_t)stream, x, w, add, y, B, H, W, C, kh, kw, dil, flip, dtype);
  return check_launch(what);
}

// partial rows of the weight gradient: H rows of nchunk workgroups, about 1024 workgroups per launch
int wgrad_chunks(int B, int H, const Geo& g) {
  long long n = (1024 + (long long)g.gx * H - 1) / ((long long)g.gx * H);
  const long long items = (long long)B * g.tiles;
  if (n > items) n = items;
  if (n > 65535) n = 65535;
  return (int)(n < 1 ? 1 : n);
}

// grid of a pass over [rows][C]: (channel blocks, row blocks), `per` rows per thread, at most `cap` row blocks
struct RowGrid {
  int lcw;
  dim3 grid;
};
RowGrid row_grid(long long rows, int C, int dtype, int per, int cap) {
  const int dv = C / (dtype == HTRVT_BF16 ? 8 : 4);
  RowGrid r;
  r.lcw = 0;
  while ((1 << r.lcw) < dv && r.lcw < 5) ++r.lcw;
  const long long rpb = (long long)per * (NT >> r.lcw);
  long long gy = (rows + rpb - 1) / rpb;
  gy = gy < 1 ? 1 : (gy > cap ? cap : gy);
  r.grid = dim3((dv + (1 << r.lcw) - 1) >> r.lcw, (unsigned)gy);
  return r;
}

template <int MODE>
int ew_entry(const char* what, const void* a, const void* b, const void* c, const float* scale, const float* shift, void* o1,
             void* o2, long long rows, int C, int dtype, void* stream) {
  if (check_rows(what, rows, C, dtype)) return -1;
  HTRVT_REQUIRE(!misaligned16(a, b, c, o1, o2), "%s: a tensor is not 16-byte aligned", what);
  const RowGrid g = row_grid(rows, C, dtype, 4, 16384);
  if (dtype == HTRVT_BF16)
    hipLaunchKernelGGL((ew_kernel<bf16_t, MODE>), g.grid, dim3(NT), 0, (hipStream_t)stream, (const bf16_t*)a, (const bf16_t*)b,
                       (const bf16_t*)c, scale, shift, (bf16_t*)o1, (bf16_t*)o2, rows, C, g.lcw);
  else
    hipLaunchKernelGGL((ew_kernel<float, MODE>), g.grid, dim3(NT), 0, (hipStream_t)stream, (const float*)a, (const float*)b,
                       (const float*)c, scale, shift, (float*)o1, (float*)o2, rows, C, g.lcw);
  return check_launch(what);
}

template <bool FWD>
int hpool_entry(const char* what, const void* in, void* out, int B, int H, int W, int C, int dtype, void* stream) {
  HTRVT_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: B=%d H=%d W=%d", what, B, H, W);
  HTRVT_REQUIRE((long long)B * H * W < (1ll << 31), "%s: too many pixels", what);
  const long long rows = (long long)B * W;
  if (check_rows(what, rows, C, dtype)) return -1;
  HTRVT_REQUIRE(in && out, "%s: null buffer", what);
  HTRVT_REQUIRE(!misaligned16(in, out), "%s: a tensor is not 16-byte aligned", what);
  const RowGrid g = row_grid(rows, C, dtype, 1, 16384);
  if (dtype == HTRVT_BF16)
    hipLaunchKernelGGL((hpool_kernel<bf16_t, FWD>), g.grid, dim3(NT), 0, (hipStream_t)stream, (const bf16_t*)in, (bf16_t*)out,
                       rows, H, W, C, g.lcw);
  else
    hipLaunchKernelGGL((hpool_kernel<float, FWD>), g.grid, dim3(NT), 0, (hipStream_t)stream, (const float*)in, (float*)out,
                       rows, H, W, C, g.lcw);
  return check_launch(what);
}

}  // namespace

extern "C" int htrvt_van_dw_fwd(const void* x, const float* w, void* y, int B, int H, int W, int C, int kh, int kw, int dil,
                                int dtype, void* stream) {
  return conv_entry("htrvt_van_dw_fwd", x, w, nullptr, y, B, H, W, C, kh, kw, dil, 0, dtype, stream);
}

extern "C" int htrvt_van_dw_bwd_input(const void* dy, const float* w, const void* add, void* dx, int B, int H, int W, int C,
                                      int kh, int kw, int dil, int dtype, void* stream) {
  return conv_entry("htrvt_van_dw_bwd_input", dy, w, add, dx, B, H, W, C, kh, kw, dil, 1, dtype, stream);
}

extern "C" int htrvt_van_dw_rows(int B, int H, int W, int C, int kh, int kw, int dil, int dtype) {
  if (check_conv("htrvt_van_dw_rows", B, H, W, C, kh, kw, dil, dtype)) return -1;
  return H * wgrad_chunks(B, H, make_geo(W, C, kh, kw, dil, dtype));
}

extern "C" int64_t htrvt_van_dw_bwd_workspace_floats(int B, int H, int W, int C, int kh, int kw, int dil, int dtype) {
  const int rows = htrvt_van_dw_rows(B, H, W, C, kh, kw, dil, dtype);
  return rows < 0 ? -1 : (int64_t)rows * C * kh * kw;
}

extern "C" int htrvt_van_dw_bwd_weight(const void* x, const void* dy, float* partial, int B, int H, int W, int C, int kh, int kw,
                                       int dil, int dtype, void* stream) {
  const char* what = "htrvt_van_dw_bwd_weight";
  if (check_conv(what, B, H, W, C, kh, kw, dil, dtype)) return -1;
  HTRVT_REQUIRE(x && dy && partial, "%s: null buffer", what);
  HTRVT_REQUIRE(!misaligned16(x, dy), "%s: a tensor is not 16-byte aligned", what);
  const Geo g = make_geo(W, C, kh, kw, dil, dtype);
  const dim3 grid(g.gx, wgrad_chunks(B, H, g), H);
#define LAUNCH(KK)                                                                                                       \
  do {                                                                                                                   \
    if (dtype == HTRVT_BF16)                                                                                             \
      hipLaunchKernelGGL((dw_wgrad_kernel<bf16_t, KK>), grid, dim3(NT), 0, (hipStream_t)stream, (const bf16_t*)x,        \
                         (const bf16_t*)dy, partial, B, H, W, C, kh, dil, g.lcw, g.rc, g.tiles);                         \
    else                                                                                                                 \
      hipLaunchKernelGGL((dw_wgrad_kernel<float, KK>), grid, dim3(NT), 0, (hipStream_t)stream, (const float*)x,          \
                         (const float*)dy, partial, B, H, W, C, kh, dil, g.lcw, g.rc, g.tiles);                          \
  } while (0)
  VAN_BY_KW(kw, LAUNCH)
#undef LAUNCH
  return check_launch(what);
}

extern "C" int htrvt_van_moments_rows(int64_t rows, int C, int dtype) {
  if (check_rows("htrvt_van_moments_rows", rows, C, dtype)) return -1;
  return (int)row_grid(rows, C, dtype, 1, 128).grid.y;
}

extern "C" int htrvt_van_moments(const void* x, float* partial, int64_t rows, int C, int dtype, void* stream) {
  const char* what = "htrvt_van_moments";
  if (check_rows(what, rows, C, dtype)) return -1;
  HTRVT_REQUIRE(x && partial, "%s: null buffer", what);
  HTRVT_REQUIRE(!misaligned16(x), "%s: x is not 16-byte aligned", what);
  const RowGrid g = row_grid(rows, C, dtype, 1, 128);
  if (dtype == HTRVT_BF16)
    hipLaunchKernelGGL(moments_kernel<bf16_t>, g.grid, dim3(NT), 0, (hipStream_t)stream, (const bf16_t*)x, partial,
                       (long long)rows, C, g.lcw);
  else
    hipLaunchKernelGGL(moments_kernel<float>, g.grid, dim3(NT), 0, (hipStream_t)stream, (const float*)x, partial,
                       (long long)rows, C, g.lcw);
  return check_launch(what);
}

extern "C" int htrvt_van_gate_fwd(const void* a, const void* p, const float* scale, const float* shift, void* g, int64_t rows,
                                  int C, int dtype, void* stream) {
  HTRVT_REQUIRE(a && p && g, "htrvt_van_gate_fwd: null buffer");
  return ew_entry<EW_GATE_FWD>("htrvt_van_gate_fwd", a, p, nullptr, scale, shift, g, nullptr, rows, C, dtype, stream);
}

extern "C" int htrvt_van_gate_bwd(const void* dg, const void* a, const void* p, const float* scale, const float* shift, void* da,
                                  void* dz, int64_t rows, int C, int dtype, void* stream) {
  HTRVT_REQUIRE(dg && a && p && da && dz, "htrvt_van_gate_bwd: null buffer");
  return ew_entry<EW_GATE_BWD>("htrvt_van_gate_bwd", dg, a, p, scale, shift, da, dz, rows, C, dtype, stream);
}

extern "C" int htrvt_van_bn_res_gelu_fwd(const void* x, const float* scale, const float* shift, const void* res, void* y,
                                         int64_t rows, int C, int dtype, void* stream) {
  HTRVT_REQUIRE(x && y, "htrvt_van_bn_res_gelu_fwd: null buffer");
  return ew_entry<EW_GELU_FWD>("htrvt_van_bn_res_gelu_fwd", x, res, nullptr, scale, shift, y, nullptr, rows, C, dtype, stream);
}

extern "C" int htrvt_van_bn_res_gelu_bwd(const void* dy, const void* x, const float* scale, const float* shift, const void* res,
                                         void* dt, int64_t rows, int C, int dtype, void* stream) {
  HTRVT_REQUIRE(dy && x && dt, "htrvt_van_bn_res_gelu_bwd: null buffer");
  return ew_entry<EW_GELU_BWD>("htrvt_van_bn_res_gelu_bwd", dy, x, res, scale, shift, dt, nullptr, rows, C, dtype, stream);
}

extern "C" int htrvt_van_hpool_fwd(const void* x, void* y, int B, int H, int W, int C, int dtype, void* stream) {
  return hpool_entry<true>("htrvt_van_hpool_fwd", x, y, B, H, W, C, dtype, stream);
}

extern "C" int htrvt_van_hpool_bwd(const void* d, void* dx, int B, int H, int W, int C, int dtype, void* stream) {
  return hpool_entry<false>("htrvt_van_hpool_bwd", d, dx, B, H, W, C, dtype, stream);
}
