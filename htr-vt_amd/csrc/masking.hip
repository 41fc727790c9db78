// masking.hip -- the multi-mask forks' token masking as a stand-alone pass, for stems other than the ResNet (whose final
// max-pool applies the mask itself, htrvt_pool_tokens / htrvt_pool_tokens_ps):
//   htrvt_mask_tokens_fwd   y[r][:] = keep[r % keep_mod] != 0 ? x[r][:] : mask_token[:]
//                           (model_sgm_mms_attach/model/HTR_VT.py:377, x * keep + (1 - keep) * mask_token with keep in {0, 1})
//   htrvt_mask_tokens_bwd   dx[r][:] = keep[r % keep_mod] != 0 ? dy[r][:] : 0
// keep_mod = N: one [N] mask for every sample; keep_mod = rows = B N: a [B][N] mask, one row per sample.  The mask token's
// gradient, the sum of dy over the masked rows, is htrvt_colsum(dy, rows, D, D, out, keep, keep_mod): its row filter is
// this rule and its two-stage sum has a fixed order (no float atomics).
// HBM-bound element-wise passes: one 16-byte vector per thread and step, a grid-stride loop, no LDS.
#include "common.h"

using namespace htrvt;

namespace {

constexpr int NT = 256;

// fill == nullptr: masked rows become zero (the backward); a vector never crosses a row (D is a multiple of its elements)
template <typename T>
__global__ __launch_bounds__(NT) void mask_tokens_kernel(const T* __restrict__ x, const float* __restrict__ keep,
                                                         unsigned keep_mod, const float* __restrict__ fill,
                                                         T* __restrict__ y, long long nvec, int cvec) {
  using Raw = decltype(Vec16<T>().raw);
  constexpr int CH = Vec16<T>::N;
  for (long long v = (long long)blockIdx.x * NT + threadIdx.x; v < nvec; v += (long long)gridDim.x * NT) {
    const long long row = v / cvec;
    const int cv = (int)(v - row * cvec);
    Vec16<T> o;
    if (keep[(unsigned long long)row % keep_mod] != 0.f) {
      o.raw = reinterpret_cast<const Raw*>(x)[v];
    } else {
#pragma unroll
      for (int j = 0; j < CH; ++j) o.set(j, fill != nullptr ? fill[cv * CH + j] : 0.f);
    }
    reinterpret_cast<Raw*>(y)[v] = o.raw;
  }
}

int launch(const char* what, const void* x, const float* keep, int64_t keep_mod, const float* fill, void* y, int64_t rows,
           int D, int dtype, void* stream) {
  const int ch = dtype == HTRVT_BF16 ? 8 : 4;
  HTRVT_REQUIRE(dtype == HTRVT_BF16 || dtype == HTRVT_F32, "%s: dtype %d is neither float32 nor bfloat16", what, dtype);
  HTRVT_REQUIRE(D > 0 && D % ch == 0 && rows >= 0, "%s: %lld rows of D=%d (a multiple of %d)", what, (long long)rows, D, ch);
  if (rows == 0) return 0;
  HTRVT_REQUIRE(x && keep && y, "%s: null buffer", what);
  HTRVT_REQUIRE(keep_mod > 0 && keep_mod <= rows && rows % keep_mod == 0 && keep_mod < (1ll << 32),
                "%s: keep_mod=%lld does not divide the %lld rows", what, (long long)keep_mod, (long long)rows);
  const long long nvec = rows * (D / ch);
  long long g = (nvec + NT - 1) / NT;
  const int grid = (int)(g > 8192 ? 8192 : g);
  if (dtype == HTRVT_BF16)
    hipLaunchKernelGGL(mask_tokens_kernel<bf16_t>, dim3(grid), dim3(NT), 0, (hipStream_t)stream, (const bf16_t*)x, keep,
                       (unsigned)keep_mod, fill, (bf16_t*)y, nvec, D / ch);
  else
    hipLaunchKernelGGL(mask_tokens_kernel<float>, dim3(grid), dim3(NT), 0, (hipStream_t)stream, (const float*)x, keep,
                       (unsigned)keep_mod, fill, (float*)y, nvec, D / ch);
  return check_launch(what);
}

}  // namespace

extern "C" int htrvt_mask_tokens_fwd(const void* x, const float* keep, int64_t keep_mod, const float* mask_token, void* y,
                                     int64_t rows, int D, int dtype, void* stream) {
  HTRVT_REQUIRE(mask_token != nullptr || rows == 0, "htrvt_mask_tokens_fwd: null mask_token");
  return launch("htrvt_mask_tokens_fwd", x, keep, keep_mod, mask_token, y, rows, D, dtype, stream);
}

extern "C" int htrvt_mask_tokens_bwd(const void* dy, const float* keep, int64_t keep_mod, void* dx, int64_t rows, int D,
                                     int dtype, void* stream) {
  return launch("htrvt_mask_tokens_bwd", dy, keep, keep_mod, nullptr, dx, rows, D, dtype, stream);
}
