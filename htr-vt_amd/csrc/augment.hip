// augment.hip -- the train-time augmentation in front of the path: what the reference's collate function
// (data/dataset.py:13-45, SameTrCollate) does per image on the host -- a projective warp and the resize back
// (data/transform.py:151-224, skimage), a grey erosion / dilation with a full rectangle (transform.py:11-33, cv2) and a
// colour jitter (torchvision ColorJitter on a mode-L Pillow image) -- as three launches over the uniform uint8 batch
// [B][H][W] the model reads.  Every random draw is made on the host (htrvt_amd/augment.py: draw_plan) and arrives in a
// small device table; an image whose record is "off" is copied bit for bit.
//
//   warp   : float64 like skimage.  One thread per output pixel: the four pixels of the warped R x C image that the
//            bilinear resize reads are computed in registers (four taps of the source each), so the warped image never
//            exists.  The source image (32 ... 128 KB) stays in cache; nothing is staged.
//   morph  : exact integers.  iterations of a rows x cols rectangle = one pass with (k - 1) * it + 1 and the anchor times it
//            (what cv2 does itself for a full rectangle); separable, a row pass and a column pass over an LDS tile with halo.
//   jitter : Pillow's blend in float32, t = deg + f * (x - deg) as a rounded product and a rounded sum -- the x86-64
//            build of Pillow has no fma, so contraction is off for the whole file.
#include "common.h"

#pragma clang fp contract(off)

using namespace htrvt;

namespace {

// ------------------------------------------------------------------------------------------------------------ warp
constexpr int WT_W = 64, WT_H = 4;       // output pixels per workgroup: 64 along the row x 4 rows

__device__ __forceinline__ double src_tap(const unsigned char* s, int H, int W, int r, int c) {
  return (r >= 0 && r < H && c >= 0 && c < W) ? (double)s[(long long)r * W + c] : 255.0;   // mode='constant', cval=255, per tap
}

// pixel (r, c) of the warped image: the source at M (c, r, 1), bilinear
__device__ double warped_pixel(const unsigned char* s, const double* m, int H, int W, int r, int c) {
  const double x = (double)c, y = (double)r;
  const double u = m[0] * x + m[1] * y + m[2];
  const double v = m[3] * x + m[4] * y + m[5];
  const double q = m[6] * x + m[7] * y + m[8];
  const double sc = u / q, sr = v / q;
  if (!(fabs(sc) < 1e9 && fabs(sr) < 1e9)) return 255.0;     // not a number, or too far out for an int: every tap is outside
  const double fr = floor(sr), fc = floor(sc);
  const double dr = sr - fr, dc = sc - fc;
  const int r0 = (int)fr, c0 = (int)fc;
  const double a = src_tap(s, H, W, r0, c0), b = src_tap(s, H, W, r0, c0 + 1);
  const double cc = src_tap(s, H, W, r0 + 1, c0), d = src_tap(s, H, W, r0 + 1, c0 + 1);
  return (1.0 - dr) * ((1.0 - dc) * a + dc * b) + dr * ((1.0 - dc) * cc + dc * d);
}

__global__ __launch_bounds__(WT_W * WT_H) void aug_warp_kernel(const unsigned char* __restrict__ src,
                                                                const HtrvtAugWarp* __restrict__ table,
                                                                unsigned char* __restrict__ dst, int H, int W) {
  const int x = blockIdx.x * WT_W + (threadIdx.x % WT_W), y = blockIdx.y * WT_H + threadIdx.x / WT_W;
  if (x >= W || y >= H) return;
  const long long img = (long long)blockIdx.z * H * W;
  const unsigned char* s = src + img;
  const HtrvtAugWarp* e = table + blockIdx.z;
  const int R = e->rows, C = e->cols;
  if (!e->on || R < 1 || C < 1) {
    dst[img + (long long)y * W + x] = s[(long long)y * W + x];
    return;
  }
  double m[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) m[i] = e->m[i];
  // the resize back to H x W (order 1, grid_mode: pixel centres at + 0.5): four pixels of the warped image
  const double rr = (y + 0.5) * ((double)R / (double)H) - 0.5, cc = (x + 0.5) * ((double)C / (double)W) - 0.5;
  const double fr = floor(rr), fc = floor(cc);
  const double dr = rr - fr, dc = cc - fc;
  const int r0 = max((int)fr, 0), r1 = min((int)fr + 1, R - 1);     // clamp = 'reflect' for coordinates in (-1, R)
  const int c0 = max((int)fc, 0), c1 = min((int)fc + 1, C - 1);
  const double a = warped_pixel(s, m, H, W, r0, c0), b = warped_pixel(s, m, H, W, r0, c1);
  const double c = warped_pixel(s, m, H, W, r1, c0), d = warped_pixel(s, m, H, W, r1, c1);
  double t = (1.0 - dr) * ((1.0 - dc) * a + dc * b) + dr * ((1.0 - dc) * c + dc * d);
  t = t < 0.0 ? 0.0 : (t > 255.0 ? 255.0 : t);
  dst[img + (long long)y * W + x] = (unsigned char)(int)t;          // .astype(np.uint8): toward zero
}

// ----------------------------------------------------------------------------------------------------------- morph
constexpr int MT_H = 32, MT_W = 64, MT_NT = 256;
constexpr int MT_E = HTRVT_AUG_MAX_EXTENT;
constexpr int MT_LD = MT_W + MT_E;       // row stride of the staged tile (>= MT_W + MT_E - 1)

template <bool DILATE>
__device__ __forceinline__ unsigned char mm(unsigned char a, unsigned char b) {
  return DILATE ? (a > b ? a : b) : (a < b ? a : b);
}

// out[y][x] = min / max of in[y + dy][x + dx], dy in [-ay, re - 1 - ay], dx in [-ax, ce - 1 - ax], over the pixels inside
// the image: a pixel outside is staged as the operation's neutral value, which is the same as leaving it out
template <bool DILATE>
__global__ __launch_bounds__(MT_NT) void aug_morph_kernel(const unsigned char* __restrict__ src,
                                                           const int32_t* __restrict__ on,
                                                           unsigned char* __restrict__ dst, int H, int W, int re, int ce,
                                                           int ay, int ax) {
  __shared__ unsigned char tile[(MT_H + MT_E - 1) * MT_LD];
  __shared__ unsigned char rowm[(MT_H + MT_E - 1) * MT_W];
  const int y0 = blockIdx.y * MT_H, x0 = blockIdx.x * MT_W;
  const long long img = (long long)blockIdx.z * H * W;
  const unsigned char* s = src + img;
  unsigned char* d = dst + img;
  if (!on[blockIdx.z]) {
    for (int i = threadIdx.x; i < MT_H * MT_W; i += MT_NT) {
      const int y = y0 + i / MT_W, x = x0 + i % MT_W;
      if (y < H && x < W) d[(long long)y * W + x] = s[(long long)y * W + x];
    }
    return;
  }
  const int th = MT_H + re - 1, tw = MT_W + ce - 1;
  for (int i = threadIdx.x; i < th * tw; i += MT_NT) {
    const int r = i / tw, c = i - r * tw;
    const int gy = y0 - ay + r, gx = x0 - ax + c;
    tile[r * MT_LD + c] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? s[(long long)gy * W + gx] : (unsigned char)(DILATE ? 0 : 255);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < th * MT_W; i += MT_NT) {        // row pass
    const int r = i / MT_W, c = i % MT_W;
    unsigned char v = tile[r * MT_LD + c];
    for (int j = 1; j < ce; ++j) v = mm<DILATE>(v, tile[r * MT_LD + c + j]);
    rowm[i] = v;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < MT_H * MT_W; i += MT_NT) {      // column pass
    const int r = i / MT_W, c = i % MT_W;
    unsigned char v = rowm[i];
    for (int j = 1; j < re; ++j) v = mm<DILATE>(v, rowm[i + j * MT_W]);
    if (y0 + r < H && x0 + c < W) d[(long long)(y0 + r) * W + x0 + c] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------- jitter
constexpr int JT_NT = 1024;

// Pillow's ImagingBlend(degenerate, image, f) on one 8-bit pixel: float32, product then sum, each rounded
__device__ __forceinline__ unsigned char blend(int deg, float f, unsigned char x) {
  // plain operators under this file's contract(off): the __fmul_rn / __fadd_rn of the HIP headers are x * y and x + y
  // compiled under the headers' own contraction setting, and fuse into one fma once they are inlined here
  const float p = f * (float)((int)x - deg);
  const float t = (float)deg + p;
  if (f >= 0.0f && f <= 1.0f) return (unsigned char)(int)t;    // interpolation: inside [0, 255] already
  return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (unsigned char)(int)t);
}

// one workgroup per image: the (brightened) image's integer sum, then the two blends in the record's order
__global__ __launch_bounds__(JT_NT) void aug_jitter_kernel(const unsigned char* __restrict__ src,
                                                            const HtrvtAugJitter* __restrict__ table,
                                                            unsigned char* __restrict__ dst, int n) {
  __shared__ unsigned red[JT_NT / 64];
  const HtrvtAugJitter e = table[blockIdx.x];
  const unsigned char* s = src + (long long)blockIdx.x * n;
  unsigned char* d = dst + (long long)blockIdx.x * n;
  if (!(e.flags & HTRVT_AUG_ON)) {
    for (int i = threadIdx.x; i < n; i += JT_NT) d[i] = s[i];
    return;
  }
  const bool bright = e.flags & HTRVT_AUG_BRIGHTNESS, contrast = e.flags & HTRVT_AUG_CONTRAST;
  const bool bright_first = bright && !(e.flags & HTRVT_AUG_CONTRAST_FIRST);
  int deg = 0;
  if (contrast) {              // ImageEnhance.Contrast: int(mean + 0.5) of the image the contrast step receives
    unsigned sum = 0;          // n <= 2^24 pixels of <= 255: fits
    for (int i = threadIdx.x; i < n; i += JT_NT) sum += bright_first ? blend(0, e.brightness, s[i]) : s[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    unsigned long long total = 0;
    for (int w = 0; w < JT_NT / 64; ++w) total += red[w];
    deg = (int)((2ull * total + (unsigned long long)n) / (2ull * (unsigned long long)n));
  }
  for (int i = threadIdx.x; i < n; i += JT_NT) {
    unsigned char v = s[i];
    if (bright_first) v = blend(0, e.brightness, v);
    if (contrast) v = blend(deg, e.contrast, v);
    if (bright && !bright_first) v = blend(0, e.brightness, v);
    d[i] = v;
  }
}

int aug_geometry(const char* what, const void* src, const void* table, const void* dst, int B, int H, int W) {
  HTRVT_REQUIRE(src && table && dst, "%s: null argument", what);
  HTRVT_REQUIRE(src != dst, "%s: src and dst are the same buffer (every stage reads neighbours of the pixel it writes)", what);
  HTRVT_REQUIRE(B > 0 && B <= HTRVT_AUG_MAX_B && H > 0 && H <= HTRVT_AUG_MAX_H && W > 0 && W <= HTRVT_AUG_MAX_W,
                "%s: bad shape B=%d H=%d W=%d (caps: B <= %d, H <= %d, W <= %d)", what, B, H, W, HTRVT_AUG_MAX_B, HTRVT_AUG_MAX_H,
                HTRVT_AUG_MAX_W);
  return 0;
}

}  // namespace

extern "C" int htrvt_aug_warp(const uint8_t* src, const HtrvtAugWarp* table, uint8_t* dst, int B, int H, int W, void* stream) {
  if (aug_geometry("htrvt_aug_warp", src, table, dst, B, H, W)) return -1;
  const dim3 grid((W + WT_W - 1) / WT_W, (H + WT_H - 1) / WT_H, B);
  hipLaunchKernelGGL(aug_warp_kernel, grid, dim3(WT_W * WT_H), 0, (hipStream_t)stream, src, table, dst, H, W);
  return check_launch("aug_warp");
}

extern "C" int htrvt_aug_morph(const uint8_t* src, const int32_t* on, uint8_t* dst, int B, int H, int W, int rows, int cols,
                               int iterations, int dilate, void* stream) {
  if (aug_geometry("htrvt_aug_morph", src, on, dst, B, H, W)) return -1;
  HTRVT_REQUIRE(rows >= 1 && cols >= 1 && iterations >= 1 && rows <= MT_E && cols <= MT_E && iterations <= MT_E,
                "htrvt_aug_morph: bad element %d x %d, %d iterations", rows, cols, iterations);
  const int re = (rows - 1) * iterations + 1, ce = (cols - 1) * iterations + 1;
  HTRVT_REQUIRE(re <= MT_E && ce <= MT_E, "htrvt_aug_morph: effective element %d x %d ((k - 1) * iterations + 1) exceeds %d", re, ce,
                MT_E);
  const int ay = (rows / 2) * iterations, ax = (cols / 2) * iterations;
  const dim3 grid((W + MT_W - 1) / MT_W, (H + MT_H - 1) / MT_H, B);
  if (dilate)
    hipLaunchKernelGGL(aug_morph_kernel<true>, grid, dim3(MT_NT), 0, (hipStream_t)stream, src, on, dst, H, W, re, ce, ay, ax);
  else
    hipLaunchKernelGGL(aug_morph_kernel<false>, grid, dim3(MT_NT), 0, (hipStream_t)stream, src, on, dst, H, W, re, ce, ay, ax);
  return check_launch("aug_morph");
}

extern "C" int htrvt_aug_jitter(const uint8_t* src, const HtrvtAugJitter* table, uint8_t* dst, int B, int H, int W, void* stream) {
  if (aug_geometry("htrvt_aug_jitter", src, table, dst, B, H, W)) return -1;
  hipLaunchKernelGGL(aug_jitter_kernel, dim3(B), dim3(JT_NT), 0, (hipStream_t)stream, src, table, dst, H * W);
  return check_launch("aug_jitter");
}
