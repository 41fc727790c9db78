// sgm.hip -- the semantic-guidance (SGM) head shared by the reference's SGM forks (model_sgm_*/model/sgm_head.py), around
// the GEMM / LayerNorm / row-softmax kernels of the hot path:
//   htrvt_sgm_context      make_context_batch (:29-73): left / right windows, targets and mask built on the device
//   htrvt_sgm_query_fwd    _context_to_query (:103-110) up to txt_proj: embedding gather, mean over S, + direction token,
//                          both directions in one [B][2][L][d_txt] batch (the GEMM A operand)
//   htrvt_sgm_query_bwd    its backward: d emb per vocabulary row and d dir_left / d dir_right in a fixed order (per-chunk
//                          partial sums in LDS, then an ordered sum over the chunks; no atomics)
//   htrvt_sgm_dropout      inverted dropout with a counter-based mask keyed by (seed read from the device, element index);
//                          the backward is the same call on the gradient (the mask is regenerated, nothing is stored)
//   htrvt_sgm_xent_fwd/bwd the masked two-direction cross-entropy (:150-160): row log-softmax over V, NLL at the target,
//                          an ordered fixed-shape reduction to the scalar loss, and d logits
//   htrvt_sgm_convert      dst (+)= src between float32 / bfloat16 buffers (the model's feature tap and its gradient)
#include "common.h"
#include "dropout_common.h"

using namespace htrvt;

namespace {

constexpr int NT = 256;

inline int blocks_for(long long n, int per_block = NT, int cap = 8192) {
  long long g = (n + per_block - 1) / per_block;
  if (g > cap) g = cap;
  return (int)(g < 1 ? 1 : g);
}

template <typename T>
__device__ __forceinline__ float ld_elem(const T* p, long long i) {
  return to_f32(p[i]);
}

__device__ __forceinline__ int clamp_id(long long id, int V) { return id < 0 ? 0 : (id >= V ? V - 1 : (int)id); }

// ------------------------------------------------------------------ context batch
// table: int32 [B] offsets into ids, [B] lengths, then the packed ids.  One thread per (b, i).
__global__ __launch_bounds__(NT) void sgm_context_kernel(const int* __restrict__ table, int B, int Lmax, int S, int pad,
                                                         int bos_l, int bos_r, int eos, long long* __restrict__ left,
                                                         long long* __restrict__ right, long long* __restrict__ tgt,
                                                         float* __restrict__ mask) {
  (void)bos_r;   // in the vocabulary, but make_context_batch never emits it: right windows end in <eos>
  const long long n = (long long)B * Lmax;
  const int* ids = table + 2 * B;
  for (long long t = (long long)blockIdx.x * NT + threadIdx.x; t < n; t += (long long)gridDim.x * NT) {
    const int b = (int)(t / Lmax), i = (int)(t % Lmax);
    const int off = table[b], L = table[B + b];
    const int* seq = ids + off;
    long long* lo = left + t * S;
    long long* ro = right + t * S;
    if (i < L) {
      tgt[t] = seq[i];
      mask[t] = 1.0f;
      for (int k = 0; k < S; ++k) {
        const int j = i - S + k;            // left window ... c_{i-2}, c_{i-1}; <bos_left> where missing
        lo[k] = j >= 0 ? seq[j] : bos_l;
        const int r = i + 1 + k;            // right window c_{i+1}, c_{i+2}, ...; <eos> where missing
        ro[k] = r < L ? seq[r] : eos;
      }
    } else {
      tgt[t] = pad;
      mask[t] = 0.0f;
      for (int k = 0; k < S; ++k) {
        lo[k] = pad;
        ro[k] = pad;
      }
    }
  }
}

// ------------------------------------------------------------------ query forward
// row r = (b, dir, l) of out [B][2][L][dt]; ids from left (dir 0) / right (dir 1) [B][L][S] int64, clamped into [0, V)
template <typename T>
__global__ __launch_bounds__(NT) void sgm_query_fwd_kernel(const long long* __restrict__ left, const long long* __restrict__ right,
                                                           const float* __restrict__ emb, const float* __restrict__ dir_l,
                                                           const float* __restrict__ dir_r, T* __restrict__ out, int L, int S,
                                                           int V, int dt) {
  const long long r = blockIdx.x;
  const int b = (int)(r / (2 * L)), rem = (int)(r % (2 * L)), dir = rem / L, l = rem % L;
  const long long* ids = (dir ? right : left) + ((long long)b * L + l) * S;
  const float* dtok = dir ? dir_r : dir_l;
  const float invS = 1.0f / (float)S;
  for (int c = threadIdx.x; c < dt; c += NT) {
    float s = 0.f;
    for (int k = 0; k < S; ++k) s += emb[(long long)clamp_id(ids[k], V) * dt + c];
    out[r * dt + c] = from_f32<T>(s * invS + dtok[c]);
  }
}

// ------------------------------------------------------------------ query backward
// Stage 1: block (chunk, column group of 64): acc[V + 2][64] in LDS over the chunk's rows in order; row r adds its gradient
// to the rows of its S ids and to row V + dir.  Stage 2: ordered sum over the chunks.
constexpr int QB_ROWS = 256, QB_COLS = 64;

template <typename T>
__global__ __launch_bounds__(QB_COLS) void sgm_query_bwd_partial_kernel(const long long* __restrict__ left,
                                                                        const long long* __restrict__ right,
                                                                        const T* __restrict__ g, float* __restrict__ partial,
                                                                        long long rows, int L, int S, int V, int dt) {
  extern __shared__ float acc[];   // [V + 2][QB_COLS]
  const int t = threadIdx.x, c = blockIdx.y * QB_COLS + t;
  for (int v = 0; v < V + 2; ++v) acc[v * QB_COLS + t] = 0.f;
  const long long r0 = (long long)blockIdx.x * QB_ROWS;
  const long long r1 = r0 + QB_ROWS < rows ? r0 + QB_ROWS : rows;
  for (long long r = r0; r < r1; ++r) {
    const int b = (int)(r / (2 * L)), rem = (int)(r % (2 * L)), dir = rem / L, l = rem % L;
    const long long* ids = (dir ? right : left) + ((long long)b * L + l) * S;
    const float gv = c < dt ? ld_elem(g, r * dt + c) : 0.f;
    for (int k = 0; k < S; ++k) acc[clamp_id(ids[k], V) * QB_COLS + t] += gv;
    acc[(V + dir) * QB_COLS + t] += gv;
  }
  if (c < dt) {
    float* out = partial + (long long)blockIdx.x * (V + 2) * dt;
    for (int v = 0; v < V + 2; ++v) out[(long long)v * dt + c] = acc[v * QB_COLS + t];
  }
}

__global__ __launch_bounds__(NT) void sgm_query_bwd_final_kernel(const float* __restrict__ partial, int nchunk, int V, int dt,
                                                                 float invS, float* __restrict__ demb, float* __restrict__ ddir_l,
                                                                 float* __restrict__ ddir_r) {
  const long long n = (long long)(V + 2) * dt;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
    float s = 0.f;
    for (int k = 0; k < nchunk; ++k) s += partial[(long long)k * n + i];
    const int v = (int)(i / dt), c = (int)(i % dt);
    if (v < V) demb[i] = s * invS;
    else if (v == V) ddir_l[c] = s;
    else ddir_r[c] = s;
  }
}

// ------------------------------------------------------------------ dropout
// (the mask: dropout_common.h)
template <typename T>
__global__ __launch_bounds__(NT) void sgm_dropout_kernel(const T* __restrict__ x, T* __restrict__ y, long long nvec,
                                                         const long long* __restrict__ seed_dev, unsigned thr, float scale) {
  using Raw = decltype(Vec16<T>().raw);
  constexpr int CH = Vec16<T>::N;
  const unsigned long long seed = (unsigned long long)seed_dev[0];
  for (long long v = (long long)blockIdx.x * NT + threadIdx.x; v < nvec; v += (long long)gridDim.x * NT) {
    Vec16<T> a, o;
    a.raw = reinterpret_cast<const Raw*>(x)[v];
#pragma unroll
    for (int j = 0; j < CH; ++j) o.set(j, keep_elem(seed, v * CH + j, thr) ? a.get(j) * scale : 0.f);
    reinterpret_cast<Raw*>(y)[v] = o.raw;
  }
}

// ------------------------------------------------------------------ cross-entropy
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// logits float32 [rows][ldv], row r = (b, dir, l); one wave per row
__global__ __launch_bounds__(NT) void sgm_xent_fwd_kernel(const float* __restrict__ logits, int ldv, int V, long long rows,
                                                          int L, const long long* __restrict__ tgt, const float* __restrict__ mask,
                                                          float* __restrict__ out_l, float* __restrict__ out_r,
                                                          float* __restrict__ lse, float* __restrict__ rowloss,
                                                          double* __restrict__ rowloss64) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int b = (int)(r / (2 * L)), rem = (int)(r % (2 * L)), dir = rem / L, l = rem % L;
  const float* x = logits + r * ldv;
  float* o = dir ? out_r : out_l;        // NULL: no copy of this direction
  if (o) o += ((long long)b * L + l) * V;
  float m = -INFINITY;
  for (int c = lane; c < V; c += 64) {
    const float v = x[c];
    m = fmaxf(m, v);
    if (o) o[c] = v;
  }
  m = wave_max(m);
  float s = 0.f;
  for (int c = lane; c < V; c += 64) s += __expf(x[c] - m);
  s = wave_sum(s);
  const float ls = m + __logf(s);
  // the same row loss in float64 for the reduction: the scalar loss is then the true masked mean rounded once, whatever
  // the float32 row losses above round to
  double sd = 0.0;
  for (int c = lane; c < V; c += 64) sd += exp((double)x[c] - (double)m);
  sd = wave_sum_f64(sd);
  if (lane == 0) {
    const long long bl = (long long)b * L + l;
    const int t = clamp_id(tgt[bl], V);
    lse[r] = ls;
    rowloss[r] = (ls - x[t]) * mask[bl];
    rowloss64[r] = ((double)m + log(sd) - (double)x[t]) * (double)mask[bl];
  }
}

// loss = sum(rowloss64) / den in float64, rounded once; den = 2 max(sum(mask), 1).  One block, fixed order.
__global__ __launch_bounds__(NT) void sgm_xent_reduce_kernel(const double* __restrict__ rowloss64, long long rows,
                                                             const float* __restrict__ mask, long long nmask,
                                                             float* __restrict__ loss, float* __restrict__ den) {
  __shared__ float red[8];
  __shared__ double red64[4];
  double s = 0.0;
  float m = 0.f;
  for (long long i = threadIdx.x; i < rows; i += NT) s += rowloss64[i];
  for (long long i = threadIdx.x; i < nmask; i += NT) m += mask[i];
  s = wave_sum_f64(s);
  if ((threadIdx.x & 63) == 0) red64[threadIdx.x >> 6] = s;
  m = block_sum_256(m, red);               // its barriers also publish red64
  if (threadIdx.x == 0) {
    const float d = 2.0f * fmaxf(m, 1.0f);
    loss[0] = (float)((red64[0] + red64[1] + red64[2] + red64[3]) / (double)d);
    den[0] = d;
  }
}

// dlogits [rows][ldv] (dtype) = (softmax - onehot) * mask * g / den (+ the incoming gradient of the returned logits);
// columns V .. ldv-1 are written as zero
template <typename T>
__global__ __launch_bounds__(NT) void sgm_xent_bwd_kernel(const float* __restrict__ logits, int ldv, int V, long long rows, int L,
                                                          const long long* __restrict__ tgt, const float* __restrict__ mask,
                                                          const float* __restrict__ lse, const float* __restrict__ den,
                                                          const float* __restrict__ gout, const float* __restrict__ dl_l,
                                                          const float* __restrict__ dl_r, T* __restrict__ dlogits) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int b = (int)(r / (2 * L)), rem = (int)(r % (2 * L)), dir = rem / L, l = rem % L;
  const long long bl = (long long)b * L + l;
  const float* x = logits + r * ldv;
  const float* dext = dir ? dl_r : dl_l;
  const int t = clamp_id(tgt[bl], V);
  const float ls = lse[r];
  const float w = (gout ? gout[0] : 0.f) * mask[bl] / den[0];
  for (int c = lane; c < ldv; c += 64) {
    float d = 0.f;
    if (c < V) {
      d = (__expf(x[c] - ls) - (c == t ? 1.f : 0.f)) * w;
      if (dext) d += dext[bl * V + c];
    }
    dlogits[r * ldv + c] = from_f32<T>(d);
  }
}

// ------------------------------------------------------------------ conversion
template <typename S, typename D>
__global__ __launch_bounds__(NT) void sgm_convert_kernel(const S* __restrict__ src, D* __restrict__ dst, long long n, int acc) {
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
    float v = to_f32(src[i]);
    if (acc) v += to_f32(dst[i]);
    dst[i] = from_f32<D>(v);
  }
}

}  // namespace

extern "C" int htrvt_sgm_context(const int32_t* table, int B, int Lmax, int S, int pad_id, int bos_left_id, int bos_right_id,
                                 int eos_id, int64_t* left, int64_t* right, int64_t* tgt, float* mask, void* stream) {
  HTRVT_REQUIRE(B >= 0 && Lmax >= 0 && S >= 1, "htrvt_sgm_context: B=%d Lmax=%d S=%d", B, Lmax, S);
  if ((long long)B * Lmax == 0) return 0;
  HTRVT_REQUIRE(table && left && right && tgt && mask, "htrvt_sgm_context: null buffer");
  hipLaunchKernelGGL(sgm_context_kernel, dim3(blocks_for((long long)B * Lmax)), dim3(NT), 0, (hipStream_t)stream, table, B,
                     Lmax, S, pad_id, bos_left_id, bos_right_id, eos_id, (long long*)left, (long long*)right, (long long*)tgt,
                     mask);
  return check_launch("sgm_context");
}

extern "C" int htrvt_sgm_query_fwd(const int64_t* left, const int64_t* right, const float* emb, const float* dir_left,
                                   const float* dir_right, void* out, int B, int L, int S, int V, int d_txt, int dtype,
                                   void* stream) {
  HTRVT_REQUIRE(B >= 0 && L >= 0 && S >= 1 && V >= 1 && d_txt >= 1, "htrvt_sgm_query_fwd: bad sizes");
  const long long rows = 2ll * B * L;
  if (rows == 0) return 0;
  HTRVT_REQUIRE(rows < (1ll << 31), "htrvt_sgm_query_fwd: too many rows");
  if (dtype == HTRVT_BF16)
    hipLaunchKernelGGL(sgm_query_fwd_kernel<bf16_t>, dim3((unsigned)rows), dim3(NT), 0, (hipStream_t)stream,
                       (const long long*)left, (const long long*)right, emb, dir_left, dir_right, (bf16_t*)out, L, S, V, d_txt);
  else
    hipLaunchKernelGGL(sgm_query_fwd_kernel<float>, dim3((unsigned)rows), dim3(NT), 0, (hipStream_t)stream,
                       (const long long*)left, (const long long*)right, emb, dir_left, dir_right, (float*)out, L, S, V, d_txt);
  return check_launch("sgm_query_fwd");
}

extern "C" int64_t htrvt_sgm_query_bwd_workspace_floats(int B, int L, int V, int d_txt) {
  const long long rows = 2ll * B * L;
  const long long nchunk = (rows + QB_ROWS - 1) / QB_ROWS;
  return nchunk * (V + 2) * (long long)d_txt;
}

extern "C" int htrvt_sgm_query_bwd(const int64_t* left, const int64_t* right, const void* dq, float* workspace, float* demb,
                                   float* ddir_left, float* ddir_right, int B, int L, int S, int V, int d_txt, int dtype,
                                   void* stream) {
  HTRVT_REQUIRE(B >= 0 && L >= 0 && S >= 1 && V >= 1 && d_txt >= 1, "htrvt_sgm_query_bwd: bad sizes");
  const size_t smem = (size_t)(V + 2) * QB_COLS * sizeof(float);
  HTRVT_REQUIRE(smem <= 64 * 1024, "htrvt_sgm_query_bwd: vocabulary of %d rows too large (<= %d)", V, 64 * 1024 / 256 - 2);
  HTRVT_REQUIRE(demb && ddir_left && ddir_right, "htrvt_sgm_query_bwd: null output");
  const long long rows = 2ll * B * L;
  const long long nchunk = (rows + QB_ROWS - 1) / QB_ROWS;
  hipStream_t st = (hipStream_t)stream;
  if (nchunk > 0) {
    HTRVT_REQUIRE(workspace && nchunk < 65536, "htrvt_sgm_query_bwd: workspace missing or too many rows");
    dim3 grid((unsigned)nchunk, (unsigned)((d_txt + QB_COLS - 1) / QB_COLS));
    if (dtype == HTRVT_BF16)
      hipLaunchKernelGGL(sgm_query_bwd_partial_kernel<bf16_t>, grid, dim3(QB_COLS), smem, st, (const long long*)left,
                         (const long long*)right, (const bf16_t*)dq, workspace, rows, L, S, V, d_txt);
    else
      hipLaunchKernelGGL(sgm_query_bwd_partial_kernel<float>, grid, dim3(QB_COLS), smem, st, (const long long*)left,
                         (const long long*)right, (const float*)dq, workspace, rows, L, S, V, d_txt);
  }
  hipLaunchKernelGGL(sgm_query_bwd_final_kernel, dim3(blocks_for((long long)(V + 2) * d_txt)), dim3(NT), 0, st, workspace,
                     (int)nchunk, V, d_txt, 1.0f / (float)S, demb, ddir_left, ddir_right);
  return check_launch("sgm_query_bwd");
}

extern "C" int htrvt_sgm_dropout(const void* x, void* y, int64_t n, const int64_t* seed, float p, int dtype, void* stream) {
  HTRVT_REQUIRE(p >= 0.f && p < 1.f, "htrvt_sgm_dropout: p=%g outside [0, 1)", (double)p);
  const int ch = dtype == HTRVT_BF16 ? 8 : 4;
  HTRVT_REQUIRE(n % ch == 0, "htrvt_sgm_dropout: n=%lld not a multiple of %d", (long long)n, ch);
  if (n == 0) return 0;
  HTRVT_REQUIRE(x && y && seed, "htrvt_sgm_dropout: null buffer");
  const auto [thr, scale] = drop_rate(p);
  const long long nvec = n / ch;
  if (dtype == HTRVT_BF16)
    hipLaunchKernelGGL(sgm_dropout_kernel<bf16_t>, dim3(blocks_for(nvec)), dim3(NT), 0, (hipStream_t)stream,
                       (const bf16_t*)x, (bf16_t*)y, nvec, (const long long*)seed, thr, scale);
  else
    hipLaunchKernelGGL(sgm_dropout_kernel<float>, dim3(blocks_for(nvec)), dim3(NT), 0, (hipStream_t)stream, (const float*)x,
                       (float*)y, nvec, (const long long*)seed, thr, scale);
  return check_launch("sgm_dropout");
}

extern "C" int htrvt_sgm_xent_fwd(const float* logits, int ldv, int V, int B, int L, const int64_t* tgt, const float* mask,
                                  float* logits_l, float* logits_r, float* lse, float* rowloss, double* rowloss64,
                                  float* loss, float* den, void* stream) {
  HTRVT_REQUIRE(V >= 1 && ldv >= V && B >= 0 && L >= 0, "htrvt_sgm_xent_fwd: bad sizes");
  HTRVT_REQUIRE(loss && den, "htrvt_sgm_xent_fwd: null loss / denominator");
  const long long rows = 2ll * B * L;
  HTRVT_REQUIRE(rows == 0 || (logits && tgt && mask && lse && rowloss && rowloss64), "htrvt_sgm_xent_fwd: null buffer");
  hipStream_t st = (hipStream_t)stream;
  if (rows > 0)
    hipLaunchKernelGGL(sgm_xent_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(NT), 0, st, logits, ldv, V, rows, L,
                       (const long long*)tgt, mask, logits_l, logits_r, lse, rowloss, rowloss64);
  hipLaunchKernelGGL(sgm_xent_reduce_kernel, dim3(1), dim3(NT), 0, st, rowloss64, rows, mask, rows / 2, loss, den);
  return check_launch("sgm_xent_fwd");
}

extern "C" int htrvt_sgm_xent_bwd(const float* logits, int ldv, int V, int B, int L, const int64_t* tgt, const float* mask,
                                  const float* lse, const float* den, const float* g, const float* dlogits_l,
                                  const float* dlogits_r, void* dlogits, int dtype, void* stream) {
  HTRVT_REQUIRE(V >= 1 && ldv >= V && B >= 0 && L >= 0, "htrvt_sgm_xent_bwd: bad sizes");
  const long long rows = 2ll * B * L;
  if (rows == 0) return 0;
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (dtype == HTRVT_BF16)
    hipLaunchKernelGGL(sgm_xent_bwd_kernel<bf16_t>, grid, dim3(NT), 0, (hipStream_t)stream, logits, ldv, V, rows, L,
                       (const long long*)tgt, mask, lse, den, g, dlogits_l, dlogits_r, (bf16_t*)dlogits);
  else
    hipLaunchKernelGGL(sgm_xent_bwd_kernel<float>, grid, dim3(NT), 0, (hipStream_t)stream, logits, ldv, V, rows, L,
                       (const long long*)tgt, mask, lse, den, g, dlogits_l, dlogits_r, (float*)dlogits);
  return check_launch("sgm_xent_bwd");
}

extern "C" int htrvt_sgm_convert(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, int accumulate,
                                 void* stream) {
  HTRVT_REQUIRE(n >= 0, "htrvt_sgm_convert: n < 0");
  if (n == 0) return 0;
  HTRVT_REQUIRE(src && dst, "htrvt_sgm_convert: null buffer");
  const dim3 grid(blocks_for(n)), blk(NT);
  hipStream_t st = (hipStream_t)stream;
  const long long nn = n;
  if (src_dtype == HTRVT_BF16 && dst_dtype == HTRVT_BF16)
    hipLaunchKernelGGL((sgm_convert_kernel<bf16_t, bf16_t>), grid, blk, 0, st, (const bf16_t*)src, (bf16_t*)dst, nn, accumulate);
  else if (src_dtype == HTRVT_BF16)
    hipLaunchKernelGGL((sgm_convert_kernel<bf16_t, float>), grid, blk, 0, st, (const bf16_t*)src, (float*)dst, nn, accumulate);
  else if (dst_dtype == HTRVT_BF16)
    hipLaunchKernelGGL((sgm_convert_kernel<float, bf16_t>), grid, blk, 0, st, (const float*)src, (bf16_t*)dst, nn, accumulate);
  else
    hipLaunchKernelGGL((sgm_convert_kernel<float, float>), grid, blk, 0, st, (const float*)src, (float*)dst, nn, accumulate);
  return check_launch("sgm_convert");
}
