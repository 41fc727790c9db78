// dropout.hip -- the regularisers of a transformer block's residual branches in one pass (the forks' `x = x +
// drop_path(dropout(branch(x)))`, model_window/model/HTR_VT.py Block.forward):
//   htrvt_residual_dropout   y = res + x * keepE(i) / (1 - p) * keepS(b) / (1 - p_path)
//     keepE(i) = keep_elem(seeds[0], i, thr(p))        element-wise dropout, i the element's index in x [rows][D]
//     keepS(b) = keep_elem(seeds[1], b, thr(p_path))   drop-path: the whole branch of sample b = row / rows_per_sample
//   res == NULL: y = x * (the same factors) -- the backward (dx from dy; the residual's gradient is dy itself).
// The masks are those of dropout_common.h, regenerated from the seeds: nothing is stored between forward and backward.
#include "common.h"
#include "dropout_common.h"

using namespace htrvt;

namespace {

constexpr int NT = 256;

// one 16-byte vector per thread and step; a vector never crosses a row (D is a multiple of the vector's elements)
template <typename T>
__global__ __launch_bounds__(NT) void residual_dropout_kernel(const T* __restrict__ x, const T* __restrict__ res, T* __restrict__ y,
                                                              long long nvec, int vec_per_sample,
                                                              const long long* __restrict__ seeds, unsigned thr, unsigned thr_path,
                                                              float scale) {
  using Raw = decltype(Vec16<T>().raw);
  constexpr int CH = Vec16<T>::N;
  const unsigned long long seed = thr ? (unsigned long long)seeds[0] : 0ull;
  const unsigned long long seed_path = thr_path ? (unsigned long long)seeds[1] : 0ull;
  for (long long v = (long long)blockIdx.x * NT + threadIdx.x; v < nvec; v += (long long)gridDim.x * NT) {
    Vec16<T> a, o;
    a.raw = reinterpret_cast<const Raw*>(x)[v];
    if (res != nullptr) o.raw = reinterpret_cast<const Raw*>(res)[v];
    const float s = keep_elem(seed_path, v / vec_per_sample, thr_path) ? scale : 0.f;
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const float t = keep_elem(seed, v * CH + j, thr) ? a.get(j) * s : 0.f;
      o.set(j, res != nullptr ? o.get(j) + t : t);
    }
    reinterpret_cast<Raw*>(y)[v] = o.raw;
  }
}

}  // namespace

extern "C" int htrvt_residual_dropout(const void* x, const void* res, void* y, int rows_per_sample, int64_t n, int D,
                                      const int64_t* seeds, float p, float p_path, int dtype, void* stream) {
  HTRVT_REQUIRE(p >= 0.f && p < 1.f && p_path >= 0.f && p_path < 1.f, "htrvt_residual_dropout: p=%g / p_path=%g outside [0, 1)",
                (double)p, (double)p_path);
  const int ch = dtype == HTRVT_BF16 ? 8 : 4;
  HTRVT_REQUIRE(D > 0 && D % ch == 0 && rows_per_sample > 0 && n >= 0 && n % D == 0,
                "htrvt_residual_dropout: n=%lld elements in rows of D=%d (a multiple of %d), %d rows per sample", (long long)n, D, ch,
                rows_per_sample);
  if (n == 0) return 0;
  HTRVT_REQUIRE(x && y && (seeds || (p == 0.f && p_path == 0.f)), "htrvt_residual_dropout: null buffer");
  const DropRate e = drop_rate(p), s = drop_rate(p_path);
  const long long nvec = n / ch, vps = (long long)rows_per_sample * (D / ch);
  HTRVT_REQUIRE(vps < (1ll << 31), "htrvt_residual_dropout: sample of %lld vectors too large", vps);
  long long g = (nvec + NT - 1) / NT;
  const int grid = (int)(g > 8192 ? 8192 : g);
  const float scale = e.scale * s.scale;
  if (dtype == HTRVT_BF16)
    hipLaunchKernelGGL(residual_dropout_kernel<bf16_t>, dim3(grid), dim3(NT), 0, (hipStream_t)stream, (const bf16_t*)x,
                       (const bf16_t*)res, (bf16_t*)y, nvec, (int)vps, (const long long*)seeds, e.thr, s.thr, scale);
  else
    hipLaunchKernelGGL(residual_dropout_kernel<float>, dim3(grid), dim3(NT), 0, (hipStream_t)stream, (const float*)x,
                       (const float*)res, (float*)y, nvec, (int)vps, (const long long*)seeds, e.thr, s.thr, scale);
  return check_launch("residual_dropout");
}
