// gemm_halo.hip -- instantiations + host-side eligibility of the halo-staged 3x3 convolution kernels (gemm_halo_impl.h);
// called from gemm_dma_try_launch before the generic gather kernels.
#include <stdlib.h>

#include "gemm_halo_impl.h"

namespace {

// ---- what all three kernels ask of a descriptor, each stated once ----
// tile selector: 0 auto, 4 loader waves, 12 these kernels where eligible; 5 is the generic gather (A/B)
bool halo_tile_selected(const HtrvtGemmDesc* d) { return d->tile == 0 || d->tile == 4 || d->tile == 12; }
// one bf16 3x3 convolution with pad 1, no batch, no split-K
bool halo_conv3x3(const HtrvtGemmDesc* d) {
  return d->dtype == HTRVT_BF16 && d->kh == 3 && d->kw == 3 && d->ph == 1 && d->pw == 1 && d->batch <= 1 && d->split_k <= 1;
}
// the staged bf16 epilogue stores 16 bytes per lane
bool halo_staged_can_store(const HtrvtGemmDesc* d) {
  return (d->ldc & 7) == 0 && (d->N & 7) == 0 && (reinterpret_cast<unsigned long long>(d->C) & 15) == 0;
}
// float32 C (the split-bf16 parity path's convolutions): plain stores from the accumulators, alpha, a float32 residual where
// the kernel takes one (dgrad), per-tile column sums on the forward -- nothing else.  (relu_src / bnb_partial / relu_scale
// never arrive with a float32 C: gemm_dma_try_launch and htrvt_gemm refuse them first.)
bool halo_f32_c_plain(const HtrvtGemmDesc* d, bool residual_ok) {
  return d->colscale == nullptr && d->bias == nullptr && d->act == 0 && d->preact == nullptr && d->relu_src == nullptr &&
         d->bnb_partial[0] == nullptr && d->relu_scale == nullptr && !d->accumulate && (residual_ok || d->residual == nullptr);
}
// forward through the staged epilogue: raw output (+ BatchNorm column sums) in training, or the eval-mode fold
// C = relu?(acc * colscale + bias [+ residual]) -- both are paths of the shared staged epilogue; GELU / saved pre-activations
// do not occur on convolutions, and a residual only as part of the eval fold
bool halo_fwd_epilogue_ok(const HtrvtGemmDesc* d) {
  return d->preact == nullptr && (d->act == 0 || d->act == 3) && !(d->residual != nullptr && d->colscale == nullptr);
}

}  // namespace

namespace htrvt {

// 1 launched, 0 not served, < 0 error.  p.tiles_m / tiles_n / shifts are set by the caller for a 256 x bn tiling.
int gemm_halo_try_launch(const HtrvtGemmDesc* d, const KParams& p, int bn, hipStream_t st) {
  const bool fwd = d->gather == HTRVT_GATHER_CONV_FWD, dgr = d->gather == HTRVT_GATHER_CONV_DGRAD;
  if (!(fwd || dgr) || !halo_tile_selected(d) || !halo_conv3x3(d)) return 0;
  if (d->sw != 1 || d->cls_h >= 0) return 0;
  if (d->sh != 1 && !(fwd && d->sh == 2)) return 0;                           // forward also with a row stride of 2 (layer1.0.conv1)
  if (d->Ho != (d->Hi - 1) / d->sh + 1 || d->Wo != d->Wi || (d->Wi % 256) != 0) return 0;    // an M tile = 256 pixels of one image row
  if (d->K != 9 * d->Cpad) return 0;
  if (d->c_f32) {
    if (!halo_f32_c_plain(d, dgr)) return 0;
    if (bn == 192) return fwd ? launch_halo<192, false, true>(p, st) : launch_halo<192, true, true>(p, st);
    if (bn == 128) return fwd ? launch_halo<128, false, true>(p, st) : launch_halo<128, true, true>(p, st);
    return 0;
  }
  if (!halo_staged_can_store(d)) return 0;
  if (fwd && !halo_fwd_epilogue_ok(d)) return 0;
  if (dgr && (d->preact != nullptr || d->colscale != nullptr || d->bias != nullptr || d->act != 0)) return 0;
  if (bn == 192) return fwd ? launch_halo<192, false>(p, st) : launch_halo<192, true>(p, st);
  if (bn == 128) return fwd ? launch_halo<128, false>(p, st) : launch_halo<128, true>(p, st);
  return 0;
}

// Forward with a column stride of 2 (layer2.0 / layer3.0 conv1, stride (2,2)): odd / even pixel images (gemm_halo_fs2_kernel).
// Same return convention and caller-set tiling as gemm_halo_try_launch.
int gemm_halo_fs2_try_launch(const HtrvtGemmDesc* d, const KParams& p, int bn, hipStream_t st) {
  if (d->gather != HTRVT_GATHER_CONV_FWD || !halo_tile_selected(d) || !halo_conv3x3(d)) return 0;
  if (d->sw != 2 || (d->sh != 1 && d->sh != 2) || d->cls_h >= 0) return 0;
  if ((d->Wi & 1) || d->Wo != d->Wi / 2 || d->Ho != (d->Hi - 1) / d->sh + 1 || (d->Wo % 256) != 0) return 0;   // an M tile = 256 pixels of one output row
  if (d->K != 9 * d->Cpad || d->M != d->nB * d->Ho * d->Wo) return 0;
  if (d->c_f32) {
    if (!halo_f32_c_plain(d, false)) return 0;
    if (bn == 192) return launch_halo_fs2<192, true>(p, st);
    if (bn == 128) return launch_halo_fs2<128, true>(p, st);
    return 0;
  }
  if (!halo_staged_can_store(d) || !halo_fwd_epilogue_ok(d)) return 0;
  if (bn == 192) return launch_halo_fs2<192>(p, st);
  if (bn == 128) return launch_halo_fs2<128>(p, st);
  return 0;
}

// Merged strided dgrad (HtrvtGemmDesc.cls_h == -2): 1 launched, 0 not served, < 0 error.  Sets p.tiles_m / tiles_n / Hq / Wq.
// `probe`: only answer (tiles_m, or 0) -- htrvt_gemm_dgrad_merged_tiles
int gemm_halo_s2_try_launch(const HtrvtGemmDesc* d, KParams& p, hipStream_t st, bool probe) {
  if (d->gather != HTRVT_GATHER_CONV_DGRAD || d->cls_h != -2 || !halo_tile_selected(d) || !halo_conv3x3(d)) return 0;
  if (d->sh != 2 || (d->sw != 1 && d->sw != 2)) return 0;
  if ((d->Hi & 1) || d->Wi % d->sw || d->Ho != d->Hi / 2 || d->Wo != d->Wi / d->sw || (d->Wo % 256) != 0) return 0;
  if (d->c_f32 || d->N != d->Ci || d->M != d->nB * d->Hi * d->Wi) return 0;
  if (d->K != (9 + (d->A2 != nullptr ? 1 : 0)) * d->Cpad) return 0;
  if (!halo_staged_can_store(d) || (d->Co & 7)) return 0;
  if (d->colscale != nullptr || d->bias != nullptr || d->act != 0 || d->preact != nullptr || d->relu_scale != nullptr) return 0;
  const long long lim = (1ll << 31) - 64;
  const long long abytes = (long long)d->nB * d->Ho * d->Wo * d->Co * 2;
  if (abytes >= lim || (long long)d->N * d->ldb * 2 >= lim) return 0;
  if (d->A2 != nullptr) {
    const long long diff = (const char*)d->A2 - (const char*)d->A;
    if (diff <= 0 || diff + abytes >= lim) return 0;
  }
  const int bn = d->N <= 128 ? 128 : 192;
  p.Hq = d->Hi / 2;
  p.Wq = d->Wi / d->sw;
  p.tiles_m = 2 * d->sw * d->nB * p.Hq * (p.Wq / 256);
  p.tiles_n = (d->N + bn - 1) / bn;
  if (probe) return p.tiles_m;
  p.cls_h = p.cls_w = -1;
  p.extra_off = d->A2 != nullptr ? (unsigned)((const char*)d->A2 - (const char*)d->A) : 0u;
  return bn == 192 ? launch_halo_s2<192>(p, st) : launch_halo_s2<128>(p, st);
}

}  // namespace htrvt
