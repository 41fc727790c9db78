// dropnorm.hip -- a regularised residual add and the LayerNorm behind it in one pass, forward and backward (the
// convolutional forks' blocks, model_sgm_mms_conv/model/HTR_VT.py: every `x = x + drop_path(dropout(branch))` is followed
// by a LayerNorm):
//   htrvt_drop_add_ln_fwd     s = res + x * keepE(i) / (1 - p) * keepS(b) / (1 - p_path);  y = LayerNorm(s) * gamma + beta
//   htrvt_layernorm_bwd_drop  ds = LayerNorm backward at s (+ dres);  dxb = ds * keepE(i) / (1 - p) * keepS(b) / (1 - p_path)
// what htrvt_residual_dropout + htrvt_layernorm_fwd resp. htrvt_layernorm_bwd + htrvt_residual_dropout do in two passes
// over [rows][D].  The masks are those of dropout.hip, keys included (dropout_common.h): keepE by (seeds[0], row * D + col),
// keepS by (seeds[1], row / rows_per_sample), regenerated from the seeds in both directions.
// As the row kernels of encoder.hip / bwd.hip: one wave64 per row, 16-byte vectors, the row in registers, all loads of a
// row issued together from clamped offsets, per-block partial rows of dgamma / dbeta summed in a fixed order.
#include "common.h"
#include "dropout_common.h"
#include "rowvec.h"

using namespace htrvt;

namespace {

constexpr int NT = 256;
constexpr int MAXC = 4;  // 16-byte chunks per lane kept in registers

struct DropArgs {
  const long long* seeds;   // device int64[2]; read only where the matching threshold is non-zero
  unsigned thr, thr_path;   // an element / a sample is dropped when its 24 bits are below
  float scale;              // 1 / (1 - p) / (1 - p_path), the factor htrvt_residual_dropout uses
  int rows_per_sample;
};

// the factor of row `row`'s kept elements: 0 where drop-path drops the row's sample (wave-uniform)
__device__ __forceinline__ float row_scale(const DropArgs& d, unsigned long long seed_path, long long row, long long rows) {
  if (d.thr_path == 0) return d.scale;
  // a 64-bit division is some hundred VALU instructions per row; the usual row counts take the 32-bit one
  const long long b = rows < (1ll << 31) ? (long long)((unsigned)row / (unsigned)d.rows_per_sample) : row / d.rows_per_sample;
  return keep_elem(seed_path, b, d.thr_path) ? d.scale : 0.f;
}

// f[j] = the factor of the CH elements from element index i0 on: the hash input once, stepped by DROP_G per element;
// thr == 0 (no element-wise dropout, wave-uniform) skips the hashes
template <int CH>
__device__ __forceinline__ void chunk_factors(unsigned long long seed, long long i0, unsigned thr, float rs, float (&f)[CH]) {
  if (thr == 0) {
#pragma unroll
    for (int j = 0; j < CH; ++j) f[j] = rs;
  } else {
    unsigned long long z = hash_input(seed, (unsigned long long)i0);
#pragma unroll
    for (int j = 0; j < CH; ++j, z += DROP_G) f[j] = keep_hashed(z, thr) ? rs : 0.f;
  }
}

// ------------------------------------------------------------------ forward
// NK = ceil(D / CH / 64): 16-byte chunks per lane
template <typename T, int NK>
__global__ __launch_bounds__(NT) void drop_add_ln_fwd_kernel(const T* __restrict__ x, const T* __restrict__ res, DropArgs d,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             T* __restrict__ s_out, T* __restrict__ y,
                                                             float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                             long long rows, int D, float eps) {
  constexpr int CH = Vec16<T>::N;
  using Raw = decltype(Vec16<T>().raw);
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nchunk = D / CH;
  const unsigned long long seed = d.thr ? (unsigned long long)d.seeds[0] : 0ull;
  const unsigned long long seed_path = d.thr_path ? (unsigned long long)d.seeds[1] : 0ull;
  const float rs = row_scale(d, seed_path, row, rows);
  bool act[NK];
  int cc[NK];
  Vec16<T> vx[NK], vs[NK];
  const Raw* xr = reinterpret_cast<const Raw*>(x + row * D);
  const Raw* rr = reinterpret_cast<const Raw*>(res + row * D);
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int c = lane + 64 * k;
    act[k] = c < nchunk;
    cc[k] = act[k] ? c : 0;
    vx[k].raw = xr[cc[k]];
    vs[k].raw = rr[cc[k]];
  }
  // s as it is stored (rounded to T): the statistics and y are taken from that
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    float f[CH];
    chunk_factors<CH>(seed, row * D + (long long)cc[k] * CH, d.thr, rs, f);
#pragma unroll
    for (int j = 0; j < CH; ++j) vs[k].set(j, vs[k].get(j) + (f[j] != 0.f ? vx[k].get(j) * f[j] : 0.f));
    if (act[k]) {
      reinterpret_cast<Raw*>(s_out + row * D)[cc[k]] = vs[k].raw;
#pragma unroll
      for (int j = 0; j < CH; ++j) sum += vs[k].get(j);
    }
  }
  const float mean = wave_sum(sum) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    if (act[k]) {
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const float t = vs[k].get(j) - mean;
        q += t * t;
      }
    }
  }
  const float rstd = rsqrtf(wave_sum(q) / (float)D + eps);
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    if (act[k]) {
      float g[CH], b[CH];
      ld_coef<CH>(gamma, cc[k] * CH, 1.f, g);
      ld_coef<CH>(beta, cc[k] * CH, 0.f, b);
      Vec16<T> o;
#pragma unroll
      for (int j = 0; j < CH; ++j) o.set(j, fmaf((vs[k].get(j) - mean) * rstd, g[j], b[j]));
      reinterpret_cast<Raw*>(y + row * D)[cc[k]] = o.raw;
    }
  }
  if (lane == 0) {
    if (mean_out) mean_out[row] = mean;
    if (rstd_out) rstd_out[row] = rstd;
  }
}

// ------------------------------------------------------------------ backward
// htrvt_layernorm_bwd's kernel (bwd.hip: the same statements in the same order, so ds and partial come out the same) with
// the branch's gradient written beside ds
template <typename T, int NK>
__global__ __launch_bounds__(NT) void layernorm_bwd_drop_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                                const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                const float* __restrict__ gamma, const T* __restrict__ dres,
                                                                DropArgs d, T* __restrict__ dx, T* __restrict__ dxb,
                                                                float* __restrict__ partial, long long rows, int D) {
  constexpr int CH = Vec16<T>::N;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* red = reinterpret_cast<float*>(smem_raw);  // [4][2*D]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nchunk = D / CH;
  const unsigned long long seed = d.thr ? (unsigned long long)d.seeds[0] : 0ull;
  const unsigned long long seed_path = d.thr_path ? (unsigned long long)d.seeds[1] : 0ull;
  float ag[NK][CH], ab[NK][CH];
#pragma unroll
  for (int k = 0; k < NK; ++k)
#pragma unroll
    for (int j = 0; j < CH; ++j) ag[k][j] = ab[k][j] = 0.f;

  using Raw = decltype(Vec16<T>().raw);
  float gm[NK][CH];
  bool act[NK];
  int cc[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int c = lane + 64 * k;
    act[k] = c < nchunk;
    cc[k] = act[k] ? c : 0;
#pragma unroll
    for (int j = 0; j < CH; ++j) gm[k][j] = act[k] ? gamma[c * CH + j] : 0.f;
  }
  for (long long row = (long long)blockIdx.x * 4 + wave; row < rows; row += (long long)gridDim.x * 4) {
    const float mu = mean[row], r = rstd[row];
    const float rs = row_scale(d, seed_path, row, rows);
    Vec16<T> vx[NK], vd[NK], dr[NK];
    const Raw* xr = reinterpret_cast<const Raw*>(x + row * D);
    const Raw* dyr = reinterpret_cast<const Raw*>(dy + row * D);
    const Raw* drr = reinterpret_cast<const Raw*>(dres + row * D);
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      vx[k].raw = xr[cc[k]];
      vd[k].raw = dyr[cc[k]];
      if (dres) dr[k].raw = drr[cc[k]];
    }
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const float xh = (vx[k].get(j) - mu) * r;
        const float dd = act[k] ? vd[k].get(j) : 0.f;
        const float g = dd * gm[k][j];
        s1 += g;
        s2 += g * xh;
        ag[k][j] += dd * xh;
        ab[k][j] += dd;
      }
    }
    const float m1 = wave_sum(s1) / (float)D, m2 = wave_sum(s2) / (float)D;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      float f[CH];
      chunk_factors<CH>(seed, row * D + (long long)cc[k] * CH, d.thr, rs, f);
      Vec16<T> o, ob;
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const float xh = (vx[k].get(j) - mu) * r;
        float v = r * (vd[k].get(j) * gm[k][j] - m1 - xh * m2);
        if (dres) v += dr[k].get(j);
        o.set(j, v);
        ob.set(j, f[j] != 0.f ? v * f[j] : 0.f);
      }
      if (act[k]) {
        reinterpret_cast<Raw*>(dx + row * D)[cc[k]] = o.raw;
        reinterpret_cast<Raw*>(dxb + row * D)[cc[k]] = ob.raw;
      }
    }
  }
  // block partial of dgamma / dbeta
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int c = lane + 64 * k;
    if (c < nchunk) {
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        red[wave * 2 * D + c * CH + j] = ag[k][j];
        red[wave * 2 * D + D + c * CH + j] = ab[k][j];
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * D; i += NT)
    partial[(long long)blockIdx.x * 2 * D + i] = red[i] + red[2 * D + i] + red[4 * D + i] + red[6 * D + i];
}

// the checks both entry points share; 0, or -1 with the error set
int drop_args(const char* who, const int64_t* seeds, float p, float p_path, int rows_per_sample, int64_t rows, int D, int dtype,
              DropArgs* out) {
  HTRVT_REQUIRE(dtype == HTRVT_F32 || dtype == HTRVT_BF16, "%s: dtype %d", who, dtype);
  HTRVT_REQUIRE(p >= 0.f && p < 1.f && p_path >= 0.f && p_path < 1.f, "%s: p=%g / p_path=%g outside [0, 1)", who, (double)p,
                (double)p_path);
  const int ch = dtype == HTRVT_BF16 ? 8 : 4;
  HTRVT_REQUIRE(D > 0 && D % ch == 0 && D / ch <= 64 * MAXC, "%s: D=%d unsupported (a multiple of %d, <= %d)", who, D, ch,
                64 * MAXC * ch);
  HTRVT_REQUIRE(rows >= 0 && rows_per_sample > 0, "%s: rows=%lld, %d rows per sample", who, (long long)rows, rows_per_sample);
  HTRVT_REQUIRE(seeds || (p == 0.f && p_path == 0.f), "%s: seeds is NULL with p=%g, p_path=%g", who, (double)p, (double)p_path);
  const DropRate e = drop_rate(p), s = drop_rate(p_path);
  *out = DropArgs{(const long long*)seeds, e.thr, s.thr, e.scale * s.scale, rows_per_sample};
  return 0;
}

}  // namespace

#define DROPNORM_DISPATCH(LAUNCH)               \
  do {                                          \
    const int nk = (D / ch + 63) / 64;          \
    if (dtype == HTRVT_BF16) {                  \
      using T = bf16_t;                         \
      if (nk == 1) LAUNCH(1);                   \
      else if (nk == 2) LAUNCH(2);              \
      else if (nk == 3) LAUNCH(3);              \
      else LAUNCH(4);                           \
    } else {                                    \
      using T = float;                          \
      if (nk == 1) LAUNCH(1);                   \
      else if (nk == 2) LAUNCH(2);              \
      else if (nk == 3) LAUNCH(3);              \
      else LAUNCH(4);                           \
    }                                           \
  } while (0)

extern "C" int htrvt_drop_add_ln_fwd(const void* x, const void* res, const int64_t* seeds, float p, float p_path,
                                     int rows_per_sample, const float* gamma, const float* beta, void* s, void* y, float* mean,
                                     float* rstd, int64_t rows, int D, float eps, int dtype, void* stream) {
  DropArgs d;
  if (drop_args("htrvt_drop_add_ln_fwd", seeds, p, p_path, rows_per_sample, rows, D, dtype, &d)) return -1;
  if (rows == 0) return 0;
  HTRVT_REQUIRE(x && res && gamma && beta && s && y, "htrvt_drop_add_ln_fwd: null buffer");
  HTRVT_REQUIRE(!misaligned16((const char*)x, (const char*)res, (const char*)s, (const char*)y),
                "htrvt_drop_add_ln_fwd: x, res, s and y must be 16-byte aligned");
  HTRVT_REQUIRE((rows + 3) / 4 < (1ll << 31), "htrvt_drop_add_ln_fwd: rows=%lld too many", (long long)rows);
  const int ch = dtype == HTRVT_BF16 ? 8 : 4;
  dim3 grid((unsigned)((rows + 3) / 4));
#define FWD(NKV)                                                                                                          \
  hipLaunchKernelGGL((drop_add_ln_fwd_kernel<T, NKV>), grid, dim3(NT), 0, (hipStream_t)stream, (const T*)x, (const T*)res, d, \
                     gamma, beta, (T*)s, (T*)y, mean, rstd, (long long)rows, D, eps)
  DROPNORM_DISPATCH(FWD);
#undef FWD
  return check_launch("drop_add_ln_fwd");
}

extern "C" int htrvt_layernorm_bwd_drop(const void* dy, const void* s, const float* mean, const float* rstd, const float* gamma,
                                        const void* dres, const int64_t* seeds, float p, float p_path, int rows_per_sample,
                                        void* ds, void* dxb, float* partial, int64_t rows, int D, int dtype, void* stream) {
  DropArgs d;
  if (drop_args("htrvt_layernorm_bwd_drop", seeds, p, p_path, rows_per_sample, rows, D, dtype, &d)) return -1;
  HTRVT_REQUIRE(rows > 0, "htrvt_layernorm_bwd_drop: rows=%lld", (long long)rows);
  HTRVT_REQUIRE(dy && s && mean && rstd && gamma && ds && dxb && partial, "htrvt_layernorm_bwd_drop: null buffer");
  HTRVT_REQUIRE(!misaligned16((const char*)dy, (const char*)s, (const char*)dres, (const char*)ds, (const char*)dxb),
                "htrvt_layernorm_bwd_drop: dy, s, dres, ds and dxb must be 16-byte aligned");
  const int ch = dtype == HTRVT_BF16 ? 8 : 4;
  const size_t smem = (size_t)8 * D * 4;   // D <= 2048 floats a quarter: at most 64 KB
  dim3 grid(htrvt_layernorm_bwd_blocks(rows));
#define BWD(NKV)                                                                                                           \
  hipLaunchKernelGGL((layernorm_bwd_drop_kernel<T, NKV>), grid, dim3(NT), smem, (hipStream_t)stream, (const T*)dy, (const T*)s, \
                     mean, rstd, gamma, (const T*)dres, d, (T*)ds, (T*)dxb, partial, (long long)rows, D)
  DROPNORM_DISPATCH(BWD);
#undef BWD
  return check_launch("layernorm_bwd_drop");
}
