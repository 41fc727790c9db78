/* htrvt.h -- C ABI of libhtrvt_hip.so, the MI355X (gfx950) kernels behind the
 * HTR-VT forward / training hot path.
 *
 * The reference (0xk0ry/HTR-VT) has NO native layer and no FFI: every FLOP of
 * its hot path is an ATen call issued from model_v1/model/HTR_VT.py,
 * model_v1/model/resnet18.py and model_v1/train.py:21-30.  Each entry point
 * below therefore cites the ATen call site(s) it replaces.  The Python drop-in
 * boundary (create_model / forward) lives in htr-vt_amd/model/HTR_VT.py and
 * binds these symbols with ctypes.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer owned by
 *     the caller (PyTorch); the library allocates nothing and keeps no state.
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued on it.
 *   - return 0 on success, negative on error; htrvt_last_error() describes it.
 *   - dtype: 0 = float32, 1 = bfloat16 (storage type of activations / packed
 *     weights).  Statistics, biases, gains, master weights are always float32.
 *   - activations are NHWC ([B,H,W,C]); tokens are [B,N,D] row-major.
 */
#ifndef HTRVT_H
#define HTRVT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HTRVT_F32 0
#define HTRVT_BF16 1

#define HTRVT_KMAJOR 0  /* element (row,k) at base + row*ld + k   */
#define HTRVT_MNMAJOR 1 /* element (row,k) at base + k*ld + row   */

#define HTRVT_GATHER_NONE 0
#define HTRVT_GATHER_CONV_FWD 1   /* A rows = output pixels, K = taps*Cpad(Ci)  */
#define HTRVT_GATHER_CONV_DGRAD 2 /* A rows = input pixels,  K = taps*Cpad(Co)  */
#define HTRVT_GATHER_CONV_WGRAD 3 /* A = x gathered (MN-major, k = output pixel, M = taps*Cpad(Ci)), B = dy, N = Co */

int htrvt_version(void);
const char* htrvt_last_error(void);
/* symbol of the MFMA kernel the last htrvt_gemm call of this thread launched, spelled as rocprofv3 prints it
 * (e.g. "gemm_dma_kernel<256, 192, 0, 0, 2, 1, 2>"): lets bench.py name its roofline kernel by the profiler's symbol.
 * htrvt_error_counts records its kernel here as well, and htrvt_stem_fwd which of its three ("stem_mfma_fwd_kernel",
 * "stem_fused_fwd_kernel<bf16_t>", "stem_fused_fwd_kernel<float>"); a call that is refused leaves the value alone. */
const char* htrvt_last_kernel(void);

/* One MFMA GEMM   C[m][n] = alpha * sum_k A(m,k) * B(n,k)  (+ epilogue).
 * Replaces: nn.Linear / torch.matmul (HTR_VT.py:22,29-37,170; timm Mlp fc1/fc2),
 * F.conv2d 3x3 / 1x1 (resnet18.py:6-7,26-31,59-63) as implicit GEMM over NHWC,
 * and their autograd backward (train.py:123). */
typedef struct HtrvtGemmDesc {
  int32_t dtype;            /* element type of A and B (and of C unless c_f32)      */
  int32_t a_layout, b_layout;
  int32_t gather;
  int32_t M, N, K;
  int64_t lda, ldb, ldc;    /* in elements                                          */
  int32_t batch, batch_inner; /* batch index z -> (z / batch_inner, z % batch_inner) */
  int64_t sA_o, sA_i, sB_o, sB_i, sC_o, sC_i; /* batch strides in elements          */
  int32_t split_k;          /* >1: grid.z splits K, result accumulated (needs accumulate=1, c_f32=1) */
  /* split_k > 1 only.  NULL: the K ranges meet in C through float atomics (summation order = arrival order).
   * Non-NULL: float32 scratch of split_k*M*N elements; every K range stores its own [M][N] slab with plain stores and a
   * second launch adds the slabs into C in ascending K order -- bitwise reproducible (the float32 parity path). */
  float* splitk_ws;
  /* conv geometry (gather != 0) */
  int32_t nB, Hi, Wi, Ci, Ho, Wo, Co, kh, kw, sh, sw, ph, pw, Cpad;
  /* HTRVT_GATHER_CONV_DGRAD of a strided conv, one launch per input-pixel parity class (bfloat16 only):
   * cls_h/cls_w in [0,sh)/[0,sw) select the pixels hi%sh==cls_h, wi%sw==cls_w (M = their count, row-major over
   * (b, hi/sh, wi/sw)); K = (#taps that can reach this class) * Cpad (may be 0).  cls_h = -1: all pixels/taps.
   * cls_h = cls_w = -2: ALL parity classes of a 3x3 pad-1 stride-(2,1) / (2,2) convolution in ONE launch on halo-staged
   * tiles (csrc/gemm_halo_impl.h: gemm_halo_s2_kernel; resnet18.py:26 with stride from :59-63): M = nB*Hi*Wi, K = 9 * Cpad
   * (10 * Cpad with A2, which then rides with the class-(0,0) tiles), the epilogue / side inputs address C rows as NHWC
   * pixels, bnb_partial gets one row per (class, 256-pixel segment) tile in grid order.  Served only where
   * htrvt_gemm_dgrad_merged_tiles() says so (Hi even, Wo a multiple of 256, operands inside 2 GiB). */
  int32_t cls_h, cls_w;
  /* Parity-class dgrad of class (0, 0) only, or NULL: A2 = the gradient of the block's 1x1 downsample convolution output
   * (resnet18.py:59-63: same stride, padding 0, same [B,Ho,Wo,Co] shape as A, allocated BEHIND A within 2 GiB).  Its
   * input gradient lands on exactly the class-(0,0) pixels, through the pixel the centre tap of the 3x3 reaches, so it is
   * contracted as ONE MORE TAP: K = (#taps of the class + 1) * Cpad, and B holds kh*kw + 1 taps per row (ldb =
   * (kh*kw + 1) * Cpad), the last one the packed 1x1 weight.  Replaces a separate 1x1 dgrad (one launch per class, three
   * of them without a single tap) plus a residual round trip of the whole input gradient. */
  const void* A2;
  /* epilogue */
  float alpha;
  int32_t act;              /* 0 none, 1 exact-erf GELU, 2 multiply by GELU'(preact), 3 ReLU applied last (after residual) */
  int32_t c_f32;            /* 1: C (and residual) are float32 regardless of dtype  */
  int32_t accumulate;       /* 1: atomicAdd into float32 C                           */
  int32_t tile;             /* 0 auto; else BM*1000+BN of a built instantiation     */
  const float* bias;        /* [N] or NULL                                           */
  const float* colscale;    /* [N] or NULL: C = alpha*acc*colscale[n] + bias[n] (eval-mode BatchNorm folded into the conv) */
  void* preact;             /* same shape/type as C: value before `act`, or NULL     */
  const void* residual;     /* same shape/type as C, added last, or NULL             */
  float* colstats;          /* [ceil(M/BM)][2][N]: per-M-tile column sum / sum of squares of the
                               float accumulators (before bias), or NULL           */
  /* bfloat16 conv-dgrad outputs only (LDS-DMA kernel with loader waves, N tile 192/128/64):
   * relu_src: same shape/type as C; C = (relu_src > 0) ? value : 0, applied after `residual` (backward of ReLU).
   * bnb_*[t], t = 0,1: BatchNorm-backward sums of the (masked) gradient written to C against up to two raw conv
   * outputs bnb_x[t] (same shape as C): bnb_partial[t][bnb_tile0 + m_tile][2][N] = { sum g, sum g*(x-mean)*rstd }.
   * bnb_partial[0] == NULL disables it.
   * relu_scale / relu_shift (float32 [N], both or neither; with bnb_partial[0] set, bnb_partial[1], residual and relu_src
   * NULL): the ReLU whose backward this is was applied to BatchNorm(bnb_x[0]) -- conv -> bn1 -> relu -> conv2 inside a
   * BasicBlock, resnet18.py:27-31 -- so its mask is recomputed from the BatchNorm input the epilogue reads anyway:
   * C = (bnb_x[0] * relu_scale[n] + relu_shift[n] > 0) ? value : 0, the same fused multiply-add htrvt_bn_apply formed in
   * the forward.  Saves the read of the activation tensor (403 MB per layer-1 launch). */
  const void* relu_src;
  const void* bnb_x[2];
  const float* bnb_mean[2];
  const float* bnb_rstd[2];
  float* bnb_partial[2];
  int32_t bnb_tile0;
  const float* relu_scale;
  const float* relu_shift;
  /* 1: relu_src is a BIT mask instead of the activation itself -- bit (m * ldc + n) of the byte array, i.e. one byte per
   * 8 consecutive columns of a row, set where the ReLU's output was positive (htrvt_bn_apply_mask writes it in the forward
   * pass): 1/16 of the side-input bytes of the fused dgrad epilogue (403 -> 25 MB per layer-1 launch) */
  int32_t relu_bits;
  const void* A;
  const void* B;
  void* C;
} HtrvtGemmDesc;

int htrvt_gemm(const HtrvtGemmDesc* d, void* stream);
/* rows of colstats (= number of M tiles) the call above will write for this desc */
int htrvt_gemm_num_mtiles(const HtrvtGemmDesc* d);
/* Weight-gradient launches (gather = HTRVT_GATHER_CONV_WGRAD; or gather = 0 with both operands MN-major and float32 output: a
 * Linear weight gradient, 256 x 256 tiles when the MN-major 8-phase kernel serves it): which tiling htrvt_gemm would use.  Returns the number of
 * workgroups per K range and the tile extents when the halo-staged kernel (3x3, W stride 1, row length a multiple of 64,
 * Cpad a multiple of 64, float32 output, operands inside 2 GiB) serves the descriptor, 0 when the generic kernels do: the
 * caller's split-K choice must count the workgroups of the kernel that actually runs. */
int htrvt_gemm_wgrad_tiling(const HtrvtGemmDesc* d, int* tile_rows, int* tile_cols);
/* Merged strided dgrad (cls_h = cls_w = -2 above): the number of M tiles (= rows every bnb_partial buffer needs) when
 * htrvt_gemm serves the descriptor in that form, 0 when the caller has to launch one parity class at a time. */
int htrvt_gemm_dgrad_merged_tiles(const HtrvtGemmDesc* d);

/* ---- stem helpers (resnet18.py:42-84, HTR_VT.py:134-136,224-227) ------------- */
/* per-image mean / rstd of the raw image (param-free LayerNorm, eps 1e-5): stats[b] = {mean, rstd}.
 * img_u8 (here and in the conv1 entry points): 0 = float32 pixels; 1 = uint8 pixels taken as value / 255, i.e. the
 * torchvision ToTensor hand-off of the reference's data pipeline (data/dataset.py) fused into the first reads of the
 * image -- a quarter of the host->device bytes. */
int htrvt_img_stats(const void* img, float* stats, int B, int HW, float eps, int img_u8, void* stream);
/* conv1: whiten + 3x3 conv Cin=1 stride (2,1) pad 1 -> NHWC [B,H/2,W,C] + BN partial sums
 * colstats[B*H/2][2][C] (one row per output image row). w: [C][9] float32. */
int htrvt_conv1_fwd(const void* img, const float* stats, const float* w, void* out, float* colstats,
                    int B, int H, int W, int C, int dtype, int img_u8, void* stream);
/* Fused stem forward (resnet18.py:74-77 with HTR_VT.py:224): conv1 (one input channel) -> BatchNorm -> ReLU ->
 * max_pool2d(3, stride (2,1), pad 1) straight from the image; the conv1 tensor is never written.
 * htrvt_stem_stats: per-channel (sum, sum of squares) of the conv1 output computed from 54 second moments of the image
 *   (batch statistics of a train-mode BatchNorm without the tensor) -> colstats float32 [2][C], one partial row for
 *   htrvt_bn_finalize(rows = 1, count = B * H/2 * W); partial: float32 [htrvt_stem_stats_rows(B, H)][64] workspace.
 * htrvt_stem_fwd: y [B][Hp][W][C] in dtype (Hp = (H/2 - 1)/2 + 1), idx uint8 (arg-max 3*row + column, 15 = ReLU
 *   closed; NULL to skip) -- same values and arg-max rule as htrvt_conv1_fwd + htrvt_bn_relu_maxpool. */
int htrvt_stem_stats_rows(int B, int H);
int htrvt_stem_stats(const void* img, const float* stats, const float* w, float* partial, float* colstats, int B, int H,
                     int W, int C, int img_u8, void* stream);
int htrvt_stem_fwd(const void* img, const float* stats, const float* w, const float* scale, const float* shift, void* y,
                   uint8_t* idx, int B, int H, int W, int C, int dtype, int img_u8, void* stream);
/* BN statistics from partial sums: train mode.  partial [rows][2][C]; count = #elements per channel.
 * Writes scale = gamma*rstd, shift = beta - mean*scale, saves mean/rstd, updates running stats
 * (momentum, unbiased running_var) when running_mean != NULL and adds 1 to *num_batches_tracked (int64, may be NULL).
 * count == 1 has no unbiased variance (torch yields NaN there): running_var then takes the biased one (0).
 * rows > 256: the rows are first reduced to 64, into scratch the CALLER provides directly behind the partial rows --
 * `partial` must then be at least (rows + 64) * 2 * C floats; the 64 extra rows are overwritten. */
int htrvt_bn_finalize(const float* partial, int rows, int C, float count, const float* gamma, const float* beta,
                      float eps, float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                      float* scale, float* shift, float* save_mean, float* save_rstd, void* stream);
/* eval mode: scale/shift from running stats; rstd (may be NULL) = 1/sqrt(running_var + eps) for an eval-mode backward */
int htrvt_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                         float eps, float* scale, float* shift, float* rstd, int C, void* stream);
/* y = [relu]( x*scale+shift [+ (res*rscale+rshift | res)] ), NHWC, any number of pixels */
int htrvt_bn_apply(const void* x, const float* scale, const float* shift, const void* res, const float* rscale,
                   const float* rshift, void* y, int64_t npix, int C, int relu, int dtype, void* stream);
/* the same pass, additionally writing the ReLU bit mask of y: mask[i >> 3] bit (i & 7) = (y[i] > 0) over the flattened
 * [npix][C] output (C a multiple of 8; bfloat16 only) -- the `relu_bits` side input of the dgrad launch that takes the
 * backward of this ReLU (HtrvtGemmDesc.relu_bits), so that the backward reads 1 bit instead of 16 per element */
int htrvt_bn_apply_mask(const void* x, const float* scale, const float* shift, const void* res, const float* rscale,
                        const float* rshift, void* y, uint8_t* mask, int64_t npix, int C, int relu, int dtype, void* stream);
/* y = maxpool3x3 stride (2,1) pad 1 ( relu(x*scale+shift) ), NHWC; scale==NULL: plain maxpool of x.
 * idx (uint8 per output element, window position 0..8 of the FIRST maximum in scan order, as ATen) or NULL */
int htrvt_bn_relu_maxpool(const void* x, const float* scale, const float* shift, void* y, uint8_t* idx,
                          int B, int H, int W, int C, int dtype, void* stream);
/* tokens[b][n][:] = (keep[n] ? maxpool(x)[b,0,n,:] : mask_token) + pos[n][:];  x NHWC [B,H(<=3),N,D] */
int htrvt_pool_tokens(const void* x, const float* keep, const float* mask_token, const float* pos, void* tok,
                      int B, int H, int N, int D, int dtype, void* stream);
/* the same with one mask row per sample (the multi-mask forks' x * keep + (1 - keep) * mask_token with keep [B, L, 1],
 * model_sgm_mms_attach/model/HTR_VT.py:368-377): sample b, token n reads keep[b * keep_ld + n].  keep_ld = N: keep is
 * float32 [B][N]; keep_ld = 0: the shared [N] mask, bitwise htrvt_pool_tokens (same kernel).  Other strides are refused. */
int htrvt_pool_tokens_ps(const void* x, const float* keep, int keep_ld, const float* mask_token, const float* pos,
                         void* tok, int B, int H, int N, int D, int dtype, void* stream);

/* ---- stand-alone token masking (csrc/masking.hip), for stems that do not end in htrvt_pool_tokens ---------------
 * ATen: y = x * keep + (1 - keep) * mask_token, keep in {0, 1} (HTR_VT.py:377 of the mms forks; svtr.py masks at D = 64).
 * x, y [rows][D] float32 / bfloat16 (D a multiple of 4 / 8), mask_token float32 [D], keep float32 [keep_mod]: row r is
 * kept where keep[r % keep_mod] != 0 (keep_mod = N: one [N] mask for the batch; keep_mod = rows = B N: a [B][N] mask).
 * Backward: dx = dy where kept, 0 where masked; d mask_token[D] += sum of dy over the masked rows is
 * htrvt_colsum(dy, rows, D, D, out, keep, keep_mod, ...) -- the same row rule, a fixed summation order, no float atomics. */
int htrvt_mask_tokens_fwd(const void* x, const float* keep, int64_t keep_mod, const float* mask_token, void* y,
                          int64_t rows, int D, int dtype, void* stream);
int htrvt_mask_tokens_bwd(const void* dy, const float* keep, int64_t keep_mod, void* dx, int64_t rows, int D, int dtype,
                          void* stream);

/* ---- encoder helpers (HTR_VT.py:27-39,68-83,169-170,236-239) ------------------ */
int htrvt_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                        int64_t rows, int D, float eps, int dtype, void* stream);
/* row softmax of float32 scores [rows][n] -> probabilities of type dtype in `p`.  bias (may be NULL): float32
 * [bias_rows][n] added to the scores first, score row r taking bias row r % bias_rows (rows ordered [batch][head][query]
 * with bias_rows = heads * N: the relative-position / window bias of SURVEY 8(f-4)). */
int htrvt_softmax_rows(const float* s, void* p, int64_t rows, int n, int dtype, const float* bias, int64_t bias_rows,
                       void* stream);
/* Fused multi-head self-attention, bfloat16 (HTR_VT.py:27-36: softmax(q k^T * scale) v and its autograd backward).
 * qkv [B*N][3][heads][hd] (the qkv Linear's output), out / dout [B*N][heads][hd], dqkv like qkv; scores and
 * probabilities stay on chip.  lse2 [B*heads][N] float32 (may be NULL in the forward when no backward follows):
 * log2 of the softmax denominator in the scaled base-2 domain, P = exp2(S * scale * log2(e) - lse2).
 * delta [B*heads][N] float32: scratch of the backward (rowsum(dout * out), written by its first launch).
 * htrvt_attn_supported: any N >= 32 (partial last query / key tiles are masked inside the kernels), hd in {32, 64, 128},
 * dtype bfloat16 (others: the htrvt_gemm + htrvt_softmax_rows path).
 * bias (may be NULL): float32 [heads][N][N] added to the scaled scores before the softmax -- the variant blocks of
 * relative-position bias table gathered per (query, key) and, for 1-D windowed / shifted attention, a
 * large negative number (-1e30, not -inf) outside the query's window (model_window/model/HTR_VT.py:23-56,113-154);
 * dbias (NULL exactly when bias is NULL): float32 [heads][N][N] += sum over the batch of d(loss)/d(score) (float atomics). */
int htrvt_attn_supported(int N, int hd, int dtype);
int htrvt_attn_fwd(const void* qkv, const float* bias, void* out, float* lse2, int B, int N, int heads, int hd, float scale,
                   int dtype, void* stream);
int htrvt_attn_bwd(const void* qkv, const float* bias, const void* out, const void* dout, const float* lse2, float* delta,
                   void* dqkv, float* dbias, int B, int N, int heads, int hd, float scale, int dtype, void* stream);
/* param-free LN over all N*C logits of a sample (HTR_VT.py:136,239): in dtype -> out float32 */
int htrvt_seq_whiten_fwd(const void* x, float* y, float* stats, int B, int NC, float eps, int dtype, void* stream);

/* ---- fused log-softmax + CTC (train.py:21-30; ATen ctc_loss with cuDNN off) ---- */
/* logits [B][T][C] float32; targets concatenated int32; tgt_len/tgt_off [B] int32.
 * nll[b] (0 if infeasible, zero_infinity); grad[b][t][c] = grad_scale * d(mean_b nll)/dlogits (NULL to skip;
 * grad_scale = 1/world_size folds the data-parallel gradient average into the loss).
 * workspace: float32, htrvt_ctc_workspace_floats(B, T, max_target_len) elements (alpha, beta, frame log-sum-exp).
 * Targets of up to 127 labels: frame log-sum-exp, the alpha and beta recursions side by side (one wave each per
 * sample), then the gradient of all (b, t) rows in parallel; longer targets: one workgroup per sample. */
size_t htrvt_ctc_workspace_floats(int B, int T, int max_target_len);
int htrvt_ctc_loss(const float* logits, const int32_t* targets, const int32_t* tgt_len, const int32_t* tgt_off,
                   float* nll, float* grad, float* workspace, int B, int T, int C, int max_target_len,
                   float grad_scale, void* stream);

/* ---- backward of the path (autograd of HTR_VT.py:222-241, train.py:123) -------- */
/* Every parameter-gradient output below is float32 and is ACCUMULATED (+=). */
/* dx = rstd*(dy - mean(dy) - y*mean(dy*y)) per sample over its N*C logits; dx has type dtype and row
 * stride ldo >= C (pad columns are left untouched) */
int htrvt_seq_whiten_bwd(const float* dy, const float* y, const float* stats, void* dx, int B, int N, int C, int ldo,
                         int dtype, void* stream);
/* LayerNorm backward: dx = LN'(dy) [+ dres]; partial[blocks][2][D] = per-block {dgamma, dbeta} */
int htrvt_layernorm_bwd_blocks(int64_t rows);
int htrvt_layernorm_bwd(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma,
                        const void* dres, void* dx, float* partial, int64_t rows, int D, int dtype, void* stream);
/* dS = scale * P * (dP - rowsum(dP*P)) ; P, dS of type dtype, dP float32 */
int htrvt_softmax_bwd_rows(const void* p, const float* dp, void* ds, int64_t rows, int n, float scale, int dtype,
                           void* stream);
/* out[c] += sum_r x[r*ld + c]; rows with keep[r % keep_mod] != 0 are skipped when keep != NULL.  Reproducible
 * two-stage sum (no float atomics): workspace = htrvt_colsum_workspace_floats(rows, cols) floats (may be 0 -> NULL). */
size_t htrvt_colsum_workspace_floats(int64_t rows, int cols);
int htrvt_colsum(const void* x, int64_t rows, int cols, int64_t ld, float* out, const float* keep, int keep_mod,
                 int dtype, float* workspace, void* stream);
int htrvt_rowsum_f32(const float* partial, int rows, int cols, float* out, void* stream);
/* train-mode BatchNorm backward (resnet18.py:27-37 under autograd): g = dy * (yact > 0) when yact != NULL */
int htrvt_bn_bwd_blocks(int64_t npix);
int htrvt_bn_bwd_reduce(const void* dy, const void* yact, const void* x, const float* mean, const float* rstd,
                        float* partial, int64_t npix, int C, int dtype, void* stream);
/* count = elements per channel (train mode: batch statistics).  count <= 0: eval-mode BatchNorm, mean / rstd are the
 * running statistics (constants): same dgamma / dbeta, dx = gamma * rstd * g. */
int htrvt_bn_bwd_finalize(const float* partial, int rows, int C, float count, const float* gamma, const float* mean,
                          const float* rstd, float* dgamma, float* dbeta, float* coef /* [3][C] */, void* stream);
int htrvt_bn_bwd_apply(const void* dy, const void* yact, const void* x, const float* coef, void* dx, void* gout,
                       int64_t npix, int C, int dtype, void* stream);
/* two BatchNorms fed by the same (already masked) gradient g -- bn2 and the downsample BN of a stage's first block,
 * resnet18.py:33-37: dx1 = BN1-backward(g, x1), dx2 = BN2-backward(g, x2) with one read of g */
int htrvt_bn_bwd_apply2(const void* g, const void* x1, const float* coef1, void* dx1, const void* x2, const float* coef2,
                        void* dx2, int64_t npix, int C, int dtype, void* stream);
/* backward of htrvt_bn_relu_maxpool: g = d(bn output, ReLU-masked), x = raw conv output [B,H,W,C]: dpool scattered through
 * the arg-max bytes (a byte outside 0..8, e.g. 15, passes nothing), then zeroed where x*scale+shift <= 0.
 * scale == NULL (shift ignored): backward of the plain max-pool, no mask. */
int htrvt_maxpool_bwd(const void* dpool, const uint8_t* idx, const void* x, const float* scale, const float* shift,
                      void* g, int B, int H, int W, int C, int dtype, void* stream);
/* backward of htrvt_pool_tokens w.r.t. x (masked tokens pass no gradient) */
int htrvt_pool_tokens_bwd(const void* dtok, const void* x, const float* keep, void* dx, int B, int H, int N, int D,
                          int dtype, void* stream);
/* backward of htrvt_pool_tokens_ps: keep[b * keep_ld + n], keep_ld = N or 0 (0: bitwise htrvt_pool_tokens_bwd); both the
 * general kernel and the H == 2 kernel take the stride */
int htrvt_pool_tokens_bwd_ps(const void* dtok, const void* x, const float* keep, int keep_ld, void* dx, int B, int H,
                             int N, int D, int dtype, void* stream);
/* dW[C][9] += sum_pix dY * whitened-input tap (autograd of htrvt_conv1_fwd); partial: [blocks][C*9] float32 scratch */
int htrvt_conv1_wgrad_blocks(int B, int H);
int htrvt_conv1_wgrad(const void* img, const float* stats, const void* dy, float* dw, float* partial,
                      int B, int H, int W, int C, int dtype, int img_u8, void* stream);

/* Backward of conv1 -> BatchNorm(train) -> ReLU -> max_pool2d(3,(2,1),1) (resnet18.py:74-77 under autograd) with
 * respect to conv1.weight [C][9], bn1.weight and bn1.bias, in one pass over the pooled gradient dpool [B,Hp,W,C] and
 * the arg-max bytes written by htrvt_bn_relu_maxpool (Cin = 1: the chain rule reduces to per-channel sums, see
 * csrc/conv1_bwd.hip).  img [B,H,W] float32, stats = htrvt_img_stats output, w = conv1.weight, mean/rstd = the batch
 * statistics saved by htrvt_bn_finalize.  partial: float32 scratch of htrvt_conv1_bwd_rows(B,H) rows x
 * htrvt_conv1_bwd_row_floats(C) floats.  dw, dgamma, dbeta accumulate.  Every shape limit (C / 16-byte vector / pick of
 * channel lanes <= 8 waves, the LDS of the image rows and of the finalize kernel) is checked before the first launch: a
 * refused call enqueues nothing. */
int htrvt_conv1_bwd_rows(int B, int H);
int htrvt_conv1_bwd_row_floats(int C);
int htrvt_conv1_bwd(const void* img, const float* stats, const void* dpool, const uint8_t* idx, const float* w,
                    const float* gamma, const float* mean, const float* rstd, float* partial, float* dw, float* dgamma,
                    float* dbeta, int B, int H, int W, int C, int dtype, int img_u8, void* stream);

/* ---- variant blocks: relative-position bias of the window-attention fork -------------------------
 * model_window/model/HTR_VT.py:23-31,45-46 (table [(2P-1)][heads] + index) and :113-154 (Block._attend: pad to a multiple
 * of the window, cyclic shift, 1-D windows, key_padding_mask) as one dense additive score bias [heads][ld][ld] for
 * htrvt_attn_fwd / htrvt_softmax_rows: table entry inside a window, -1e30 outside and in the columns N..ld-1 (sequence
 * padded for the kernels; rows N..ld-1 are don't-care queries).  window <= 0: full attention.
 * Refused (non-zero, htrvt_last_error(), nothing launched): a null pointer, N > num_patches, ld < N, shift outside [0, window),
 * window > num_patches (slot distances up to window - 1 would index outside the 2 P - 1 entries; the reference raises too).
 * _bwd: dtable[(2P-1)][heads] = gather-sum of dbias over the (query, key) pairs of each entry, fixed order, overwrites. */
int htrvt_relpos_bias_fwd(const float* table, float* bias, int N, int num_patches, int window, int shift, int heads, int ld,
                          void* stream);
int htrvt_relpos_bias_bwd(const float* dbias, float* dtable, int N, int num_patches, int window, int shift, int heads, int ld,
                          void* stream);

/* Fused bfloat16 self-attention with the relative-position bias TABLE of the window-attention fork (model_window/model/
 * HTR_VT.py:11-62,113-154), forward and backward, any N >= 32 with no padded copy (csrc/attn_relpos.hip).  qkv / out /
 * dout / dqkv / lse2 / delta as for htrvt_attn_*; table [(2P-1)][heads] float32 (P = num_patches, the parameter as stored).
 * window 0: full attention, entry (key - query) + P - 1; window ws > 0: Np = ceil(N/ws) ws, pos = (t - shift) mod Np, a
 * pair attends iff pos / ws agree and uses entry pos_key % ws - pos_query % ws + P - 1; every other pair is masked.
 * _supported: 1 if (N, hd, dtype, geometry) is served -- bfloat16, hd in {64, 128}, 32 <= N <= P <= 2048, 0 <= shift < ws
 * (shift 0 without a window; a shifted window needs N > ws) -- else 0 with the reason in htrvt_last_error().
 * _bwd: dtable (may be NULL: no table gradient) += d(loss)/d(table), float32, no atomics: per-workgroup partial rows in
 * `workspace` (htrvt_attn_relpos_bwd_workspace_floats() floats, -1 on bad geometry) summed in a fixed order -- bitwise
 * reproducible. */
int htrvt_attn_relpos_supported(int N, int hd, int dtype, int num_patches, int window, int shift);
int64_t htrvt_attn_relpos_bwd_workspace_floats(int B, int N, int heads, int num_patches, int window, int shift);
int htrvt_attn_relpos_fwd(const void* qkv, const float* table, void* out, float* lse2, int B, int N, int heads, int hd,
                          float scale, int num_patches, int window, int shift, int dtype, void* stream);
int htrvt_attn_relpos_bwd(const void* qkv, const float* table, const void* out, const void* dout, const float* lse2,
                          float* delta, void* dqkv, float* dtable, float* workspace, int B, int N, int heads, int hd,
                          float scale, int num_patches, int window, int shift, int dtype, void* stream);

/* Dropout on the attention probabilities inside the fused kernels, and the regularisers of a residual branch.
 * The mask is a pure function of a seed (an int64 on the device, as for htrvt_sgm_dropout) and the element's logical index:
 *   keep(b, head, q, k) = keep_elem(seed[0], ((b heads + head) N + q) N + k, thr(p))
 * -- what htrvt_sgm_dropout draws on a dense [B*heads][N][N] tensor with the same seed and p, so the batched-GEMM route
 * gets the same mask by applying it to P (forward) and dP (backward).  out = (softmax(S) * keep / (1 - p)) v; lse2 is that
 * of the undropped softmax.  The backward regenerates the mask: nothing but the seed is kept.
 * p in [0, 1), else an error.  p == 0 is htrvt_attn_fwd/_bwd (bias NULL) resp. htrvt_attn_relpos_fwd/_bwd, bitwise, and seed
 * may then be NULL.  htrvt_attn_dropout_*: the plain scores (no bias); _supported as htrvt_attn_supported.
 * htrvt_attn_relpos_dropout_*: the table scores, shapes as htrvt_attn_relpos_supported.
 * htrvt_residual_dropout: x, res, y [n / D][D] (dtype float32 / bfloat16, D a multiple of 4 / 8), sample b = row /
 *   rows_per_sample, seeds int64[2] on the device:
 *     y = res + x * keep_elem(seeds[0], i, thr(p)) / (1 - p) * keep_elem(seeds[1], b, thr(p_path)) / (1 - p_path)
 *   (element-wise dropout, then drop-path of the whole sample, then the residual add).  res NULL: without the add -- the
 *   backward, dx from dy.  Either probability may be 0; seeds may be NULL when both are. */
int htrvt_attn_dropout_supported(int N, int hd, int dtype);
int htrvt_attn_dropout_fwd(const void* qkv, void* out, float* lse2, int B, int N, int heads, int hd, float scale,
                           const int64_t* seed, float p, int dtype, void* stream);
int htrvt_attn_dropout_bwd(const void* qkv, const void* out, const void* dout, const float* lse2, float* delta, void* dqkv,
                           int B, int N, int heads, int hd, float scale, const int64_t* seed, float p, int dtype, void* stream);
int htrvt_attn_relpos_dropout_fwd(const void* qkv, const float* table, void* out, float* lse2, int B, int N, int heads, int hd,
                                  float scale, int num_patches, int window, int shift, const int64_t* seed, float p, int dtype,
                                  void* stream);
int htrvt_attn_relpos_dropout_bwd(const void* qkv, const float* table, const void* out, const void* dout, const float* lse2,
                                  float* delta, void* dqkv, float* dtable, float* workspace, int B, int N, int heads, int hd,
                                  float scale, int num_patches, int window, int shift, const int64_t* seed, float p, int dtype,
                                  void* stream);
int htrvt_residual_dropout(const void* x, const void* res, void* y, int rows_per_sample, int64_t n, int D, const int64_t* seeds,
                           float p, float p_path, int dtype, void* stream);

/* The regularised residual add and the LayerNorm behind it in one launch, forward and backward (csrc/dropnorm.hip): what
 * htrvt_residual_dropout + htrvt_layernorm_fwd, resp. htrvt_layernorm_bwd + htrvt_residual_dropout, do in two.  x, res, s, y,
 * dy, dres, ds, dxb [rows][D] (dtype float32 / bfloat16, 16-byte aligned), D as htrvt_layernorm_fwd/_bwd: a multiple of
 * 4 / 8, at most 1024 / 2048.  The masks and their keys are htrvt_residual_dropout's: keepE by (seeds[0], row * D + col),
 * keepS by (seeds[1], row / rows_per_sample); the same seeds give the same masks on both routes and in both directions.
 * htrvt_drop_add_ln_fwd:
 *     s = res + x * keepE / (1 - p) * keepS / (1 - p_path)         the new residual stream, stored
 *     y = LayerNorm(s) * gamma + beta, mean / rstd [rows] float32   of s AS STORED (rounded to dtype): (s, mean, rstd) is
 *                                                                   what htrvt_layernorm_bwd and the backward below take
 *   mean and rstd may be NULL.
 * htrvt_layernorm_bwd_drop:
 *     ds, partial   exactly htrvt_layernorm_bwd(dy, s, mean, rstd, gamma, dres): the gradient of the residual stream (dres
 *                   may be NULL) and the [htrvt_layernorm_bwd_blocks(rows)][2][D] partial rows of dgamma / dbeta
 *     dxb = ds * keepE / (1 - p) * keepS / (1 - p_path)             the branch's gradient, from the same registers
 * Either probability may be 0 (p == 0 skips the per-element hashes); seeds may be NULL when both are.  A probability outside
 * [0, 1), an unsupported width, a missing or misaligned buffer: an error, nothing is launched. */
int htrvt_drop_add_ln_fwd(const void* x, const void* res, const int64_t* seeds, float p, float p_path, int rows_per_sample,
                          const float* gamma, const float* beta, void* s, void* y, float* mean, float* rstd, int64_t rows,
                          int D, float eps, int dtype, void* stream);
int htrvt_layernorm_bwd_drop(const void* dy, const void* s, const float* mean, const float* rstd, const float* gamma,
                             const void* dres, const int64_t* seeds, float p, float p_path, int rows_per_sample, void* ds,
                             void* dxb, float* partial, int64_t rows, int D, int dtype, void* stream);

/* ---- weight layout helpers ----------------------------------------------------- */
/* w [Co][Ci][taps] float32 -> fwd [Co][taps][cpad_in], dgrad [Ci][taps][cpad_out] (may be NULL); pads untouched */
int htrvt_pack_conv_weight(const float* w, void* fwd, void* dgrad, int Co, int Ci, int taps, int cpad_in,
                           int cpad_out, int dtype, void* stream);
/* the same with the dgrad pack written into tap slots tap0 .. tap0+taps-1 of rows that hold row_taps taps:
 * dgrad [Ci][row_taps][cpad_out] (a 3x3 weight and its block's 1x1 downsample weight share one buffer, see A2 above) */
int htrvt_pack_conv_weight_slots(const float* w, void* fwd, void* dgrad, int Co, int Ci, int taps, int cpad_in, int cpad_out,
                                 int row_taps, int tap0, int dtype, void* stream);
/* grad [Co][Ci][taps] += packed [taps][cpad_in][Co]  (the conv-wgrad GEMM output) */
int htrvt_unpack_conv_wgrad(const float* packed, float* grad, int Co, int Ci, int taps, int cpad_in, void* stream);
int htrvt_cast_f32(const float* src, void* dst, int64_t n, int dtype, void* stream);

/* The same re-layouts as ONE launch over a table of jobs (csrc/relayout.hip): every conv / Linear weight of the model is
 * re-packed once per optimizer step and every conv weight gradient unpacked once per backward -- 47 small launches per step
 * as single-tensor calls.  Fill src / dst / kind / sizes, let htrvt_relayout_plan assign the workgroup ranges (host side),
 * copy the table to the device, then htrvt_relayout(table_dev, njobs, total) runs all jobs.  A job's fields mean what the
 * single-tensor entry point of its kind documents above / below. */
#define HTRVT_RELAYOUT_PACK_CONV 0      /* src w [d0 = Co][d1 = Ci][taps] f32 -> dst0 fwd pack, dst1 dgrad pack (either may be NULL) */
#define HTRVT_RELAYOUT_CAST_TRANSPOSE 1 /* src w [d0 = rows][d1 = cols] f32 -> dst0 [rows][cols] (may be NULL), dst1 [cols][cpad_in = ld_t] */
#define HTRVT_RELAYOUT_UNPACK_WGRAD 2   /* src packed [taps][cpad_in][d0 = Co] f32, dst0 grad [Co][d1 = Ci][taps] f32 += */
#define HTRVT_RELAYOUT_MAX_JOBS 64
typedef struct HtrvtRelayoutJob {
  const void* src;
  void* dst0;
  void* dst1;
  int kind;
  int d0, d1;
  int taps, cpad_in, cpad_out, row_taps, tap0;
  int tile0, tiles_x;     /* filled by htrvt_relayout_plan */
  int reserved_[2];
} HtrvtRelayoutJob;
int htrvt_relayout_plan(HtrvtRelayoutJob* jobs_host, int njobs);   /* returns the launch's workgroup count, < 0 on a bad job */
int htrvt_relayout(const HtrvtRelayoutJob* jobs_dev, int njobs, int total_tiles, int dtype, void* stream);
/* the same launch from a planned table in HOST memory, copied into the kernel-argument segment (no device copy of the
 * table to keep alive or to refresh when a gradient buffer moves); njobs <= HTRVT_RELAYOUT_ARG_JOBS */
#define HTRVT_RELAYOUT_ARG_JOBS 48
int htrvt_relayout_host(const HtrvtRelayoutJob* jobs_host, int njobs, int total_tiles, int dtype, void* stream);
/* Linear weight w [rows = out][cols = in] float32 -> dst [rows][cols] (may be NULL) and dst_t [cols][ld_t] = w^T in
 * `dtype` (bfloat16), columns rows .. ld_t-1 of dst_t zero: the K-major B operand of the Linear dgrad GEMM
 * dx[M][in] = dy[M][out] * w (HTR_VT.py:22-37 backward), so that forward and dgrad run the same kernel. */
int htrvt_cast_transpose_f32(const float* src, void* dst, void* dst_t, int rows, int cols, int ld_t, int dtype, void* stream);

/* ---- split-bfloat16 operands of the parity path (csrc/split.hip) -----------------------------------------------------
 * x = hi + lo + O(2^-17 |x|) with hi = bf16(x), lo = bf16(x - hi); x*w = x_hi w_hi + x_lo w_hi + x_hi w_lo + O(2^-16 |x w|)
 * is ONE bfloat16 product over a three times longer K when the operands are concatenated along K (float32 accumulate):
 * the reference's float32 Linear / conv arithmetic (HTR_VT.py:22-37,76; resnet18.py:26-31,59-63) on the bf16 matrix
 * cores at a third of their rate instead of 1/16 (the f32-input MFMA), inside BASELINE.json's 1e-3 logit gate.
 * src float32 [rows][cols] (row stride ld_src) ->
 *   cat (may be NULL unless cat_f32 / transpose): [rows][3*cols], order 0 = (hi | lo | hi) -- the activation side,
 *       order 1 = (hi | hi | lo) -- the weight side; bfloat16, or float32 holding the same bf16-exact values when cat_f32
 *       (input of htrvt_pack_conv_weight); transpose: [cols][3*rows], block j of row c = part j of src[:, c]
 *   hi, lo (may be NULL): bfloat16 [rows][cols] planes (weight gradients contract over rows: three accumulating launches) */
int htrvt_split_bf16(const float* src, int64_t rows, int cols, int64_t ld_src, void* cat, int order, int cat_f32, int transpose,
                     void* hi, void* lo, void* stream);
/* Split-bf16 strided conv dgrad (resnet18.py:26,59-63 backward): the parity-class launches of htrvt_gemm with float32 output
 * leave one dense [B][Hq][Wq][C] matrix per class (a, b) = (hi % sh, wi % sw); this interleaves them into the NHWC gradient
 * dx [B][Hi][Wi][C] (+ residual, may be NULL).  c01 / c10 / c11 may be NULL where the stride in that direction is 1. */
/* float32 element-wise steps beside the split-bf16 Linear products (which write plain float32 + bias): mode 0: out = gelu_erf(a)
 * (timm Mlp's exact-erf GELU, HTR_VT.py:76), 1: out = a * gelu_erf'(b) (its backward), 2: out = a + b (residual, HTR_VT.py:81-82).
 * The float32 path has the same steps, in the same order and with the same rounding points, inside its GEMM epilogue. */
int htrvt_elementwise_f32(const float* a, const float* b, float* out, int64_t n, int mode, void* stream);
int htrvt_class_scatter_f32(const float* c00, const float* c01, const float* c10, const float* c11, const float* residual, float* dx,
                            int B, int Hi, int Wi, int C, int sh, int sw, void* stream);

/* ---- optimizer step (train.py:94 AdamW(betas .9/.99, wd .5) as one flat launch) -- */
/* Statement order and rounding points of torch.optim.AdamW's single-tensor step; the hyper-parameters are doubles as in
 * Python, derived scalars (1 - lr*wd, 1 - beta, bias corrections, -lr/bc1) are formed in double and rounded once. */
int htrvt_adamw(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                double eps, double weight_decay, int step, void* stream);
/* The same step with its derived scalars read from DEVICE memory: a captured HIP graph bakes kernel arguments, while lr
 * (utils.update_lr_cos, train.py:115) and the step number change every iteration.  htrvt_adamw_scalars forms the
 * HTRVT_ADAMW_SCALARS floats on the host exactly as htrvt_adamw does (same doubles, same single rounding), the caller
 * copies them to `hyper_dev` in stream order before the launch / the graph replay: bit-identical to htrvt_adamw. */
#define HTRVT_ADAMW_SCALARS 8
int htrvt_adamw_scalars(double lr, double beta1, double beta2, double eps, double weight_decay, int step, float* out_host);
int htrvt_adamw_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper_dev, void* stream);

/* ---- around the path: SAM, EMA, greedy decode ---------------- */
/* out[0] = sum x^2 (deterministic two-stage); partial: htrvt_sumsq_blocks(n) floats of scratch.  With x = the flat
 * gradient buffer this is SAM._grad_norm()^2 (utils/sam.py:47-56). */
int htrvt_sumsq_blocks(int64_t n);
int htrvt_sumsq(const float* x, int64_t n, float* partial, float* out, void* stream);
/* SAM.first_step (utils/sam.py:15-27, adaptive=False): old_p = p; p += g * rho / (sqrt(norm_sq[0]) + 1e-12) */
int htrvt_sam_first_step(float* p, const float* g, float* old_p, int64_t n, float rho, const float* norm_sq, void* stream);
/* SAM.second_step's restore (utils/sam.py:31-34): p = old_p; htrvt_adamw then applies the base optimizer */
int htrvt_sam_restore(float* p, const float* old_p, int64_t n, void* stream);
/* ModelEma.update (utils/utils.py:158-173) over every state_dict entry in one launch: ema = ema*decay + (1-decay)*model
 * in float32 (int64 entries: float math, truncated on the way back).  table: device array of `count` entries. */
typedef struct HtrvtEmaEntry {
  void* ema;
  const void* model;
  int64_t numel;
  int32_t is_int64;
  int32_t pad_;
} HtrvtEmaEntry;
int htrvt_ema_update(const HtrvtEmaEntry* table, int count, int64_t max_numel, double decay, void* stream);
/* valid.py:40-42 + CTCLabelConverter.decode (utils/utils.py:72-86): out[b, 0:out_len[b]] = arg-max class per frame with
 * blanks (0), repeats and indices >= ncharacter removed.  logits [B,T,ld>=C] float32 (arg-max of the logits = arg-max of
 * their log-softmax), out [B,T] int32. */
int htrvt_ctc_greedy_decode(const float* logits, int B, int T, int C, int64_t ld, int ncharacter, int32_t* out,
                            int32_t* out_len, void* stream);
/* valid.py:49-75, the metric loop: per sample b the Levenshtein distance (unit insert / delete / substitute costs) between
 * the decoded prediction and the label, over characters (editdistance.eval(pred, gt), valid.py:50) and over the word lists
 * utils.format_string_for_wer(s).split(" ") (valid.py:59-63, utils/utils.py:176-179), with the lengths CER and WER divide by.
 *   counts[b] = { ed_char, len(gt), ed_word, len(gt_words) };  totals[0:4] += their column sums (integer atomics; may be NULL).
 * pred [B][ld_pred] / pred_len [B] are htrvt_ctc_greedy_decode's out / out_len; tgt / tgt_len / tgt_off are the label arrays
 * of htrvt_ctc_loss.  Symbols are class indices; two of them are the same character iff canon[] maps them to the same value,
 * and kind[] says what a character is to the word split: 0 ordinary, 1 separator (space, newline), 2 punctuation (a word of
 * its own), 3 other white space (ordinary inside a string, dropped at its ends as str.strip does).  An index outside
 * [0, nsym) reads no table: it stands for itself and is ordinary.  A string without a word is ONE empty word, as "".split(" ")
 * is.  Words are equal iff their canonical symbols are.  One workgroup per sample, everything in LDS and registers.
 * Limits: max_pred <= 16384 (the decode's own), ld_pred >= max_pred, max_tgt <= htrvt_error_counts_max_tgt() (512).  A
 * violation, a null pointer other than totals, B <= 0 or nsym <= 0 returns a negative code before anything is launched.
 * pred_len[b] / tgt_len[b] live on the device: a value beyond max_pred / max_tgt is read as that maximum. */
int htrvt_error_counts_max_tgt(void);
int htrvt_error_counts(const int32_t* pred, int64_t ld_pred, const int32_t* pred_len, const int32_t* tgt, const int32_t* tgt_len,
                       const int32_t* tgt_off, const int32_t* canon, const uint8_t* kind, int nsym, int B, int max_pred,
                       int max_tgt, int32_t* counts, int64_t* totals, void* stream);

/* ---- in front of the path: the loader's per-image preparation -------------------------------------
 * data/dataset.py:104-135 for a ragged batch of grey uint8 scans: aspect-preserving resize to height H (npThum: width' =
 * min(int(w * H / h), W), PIL.Image.resize = Pillow's 8-bit BICUBIC resampler, restated bit for bit), img_as_float32 and
 * right pad with 1.0 -- delivered as the uint8 batch dst [B][H][W] (255 = 1.0) that the model reads as value / 255.
 * src: all scans back to back; table[i] (device) = {byte offset of scan i in src, byte offset of its scratch rows in tmp
 * (h_i * W bytes each), h_i, w_i}; max_src_h = max h_i.  Every scale factor h_i / H and w_i / width' must be
 * <= htrvt_line_max_scale() (the tap table of one output pixel is bounded); an image beyond it (or with h, w or width'
 * < 1) is delivered as an empty line, all 255, never read past the table. */
typedef struct HtrvtLineImage {
  int64_t src_offset;
  int64_t tmp_offset;
  int32_t h, w;
} HtrvtLineImage;
int htrvt_line_max_scale(void);
int htrvt_line_prepare(const uint8_t* src, const HtrvtLineImage* table, uint8_t* tmp, uint8_t* dst, int B, int H, int W,
                       int max_src_h, void* stream);

/* ---- in front of the path: the train-time augmentation (csrc/augment.hip) --------------------------------
 * data/dataset.py:13-45 (SameTrCollate): per batch three coins, and for each that lands heads one stage over every image.
 * Each stage reads the uniform uint8 batch src [B][H][W] and writes dst [B][H][W] (another buffer: src == dst is refused);
 * every random draw is made on the host and arrives in a device table; an image whose record is off is copied bit for bit.
 * Refused before any launch (-1, reason in htrvt_last_error()): a null pointer, B / H / W < 1 or above the caps below, and
 * for the morphology an effective extent above HTRVT_AUG_MAX_EXTENT.  The tables live in device memory and are not
 * read on the host: no value in them makes a kernel read or write outside the two batches.
 *
 * htrvt_aug_warp: transform.py:151-224, skimage's warp(order 1, mode 'constant', cval 255) to an R x C image and its
 *   resize(order 1, mode 'reflect') back to H x W, as one launch without the R x C image.  m = the normalised 3 x 3 map,
 *   row-major, taking pixel (c, r) of the warped image to source coordinates (u / q, v / q), (u, v, q) = m (c, r, 1).
 *   Output pixel (y, x): rr = (y + 0.5) * (R / H) - 0.5, cc likewise; floor and fraction; bilinear over four warped pixels
 *   with indices clamped to [0, R-1] x [0, C-1]; each warped pixel bilinear over four source taps, a tap outside the image
 *   = 255; both as (1-dr) * ((1-dc) * a + dc * b) + dr * ((1-dc) * c + dc * d) in float64 without fma; clamp to [0, 255],
 *   truncate.  A source point that is not finite (or beyond 1e9) reads 255.  The anti-aliasing Gaussian of a shrinking
 *   resize is left out: the host refuses plans with sigma = (R / H - 1) / 2 (or the column one) above 0.19.
 * htrvt_aug_morph: transform.py:11-33, cv2.erode / cv2.dilate with np.ones((rows, cols)), `iterations` times, one set of
 *   parameters for the batch; on int32 [B] (0 = copy).  cv2's conventions: anchor (rows / 2, cols / 2), the same offsets for
 *   both operations, pixels outside the image ignored; iterating a full rectangle = one pass with extents
 *   (k - 1) * iterations + 1 and the anchor times iterations, which is how it is run.  Exact.
 * htrvt_aug_jitter: torchvision ColorJitter on a mode-L Pillow image, where only brightness and contrast act.  Both are
 *   Pillow blends in float32, t = deg + f * (x - deg) as a rounded product then a rounded sum, truncated (0 <= f <= 1) or
 *   clipped to [0, 255] and truncated; brightness: deg = 0; contrast: deg = (2 * sum + count) / (2 * count) in integers over
 *   the image the contrast step receives (after brightness unless HTRVT_AUG_CONTRAST_FIRST).  Bit-exact against Pillow. */
#define HTRVT_AUG_MAX_B 65535
#define HTRVT_AUG_MAX_H 1024
#define HTRVT_AUG_MAX_W 16384
#define HTRVT_AUG_MAX_EXTENT 16          /* effective rows / cols of the morphology's rectangle */
typedef struct HtrvtAugWarp {
  double m[9];
  int32_t rows, cols;                    /* R, C: shape of the warped image */
  int32_t on;
  int32_t reserved_;
} HtrvtAugWarp;
#define HTRVT_AUG_ON 1                   /* HtrvtAugJitter.flags */
#define HTRVT_AUG_BRIGHTNESS 2           /* the brightness step acts (its strength is not 0) */
#define HTRVT_AUG_CONTRAST 4
#define HTRVT_AUG_CONTRAST_FIRST 8       /* the permutation puts contrast before brightness */
typedef struct HtrvtAugJitter {
  float brightness, contrast;            /* the two factors */
  int32_t flags;
  int32_t reserved_;
} HtrvtAugJitter;
int htrvt_aug_warp(const uint8_t* src, const HtrvtAugWarp* table, uint8_t* dst, int B, int H, int W, void* stream);
int htrvt_aug_morph(const uint8_t* src, const int32_t* on, uint8_t* dst, int B, int H, int W, int rows, int cols,
                    int iterations, int dilate, void* stream);
int htrvt_aug_jitter(const uint8_t* src, const HtrvtAugJitter* table, uint8_t* dst, int B, int H, int W, void* stream);

/* ---- the SGM forks' semantic-guidance head (csrc/sgm.hip; sgm_head.py of every model_sgm_ fork) ---------------------------
 * Row r of the head's query batch is (b, dir, l) of [B][2][L]: dir 0 = the left windows, 1 = the right windows.
 * htrvt_sgm_context: make_context_batch (:29-73).  table int32 = [B] offsets into the ids, [B] lengths, the packed ids;
 *   left / right int64 [B][Lmax][S], tgt int64 [B][Lmax], mask float32 [B][Lmax]; positions past a line hold pad_id / 0.
 * htrvt_sgm_query_fwd: out[r][:] (dtype) = mean over S of emb[id] + dir token (_context_to_query up to txt_proj); ids are
 *   clamped into [0, V).  _bwd: demb [V][d_txt], ddir_* [d_txt] overwritten, per-chunk LDS sums then an ordered sum over
 *   the chunks (workspace: htrvt_sgm_query_bwd_workspace_floats floats); no atomics.  V <= 254.
 * htrvt_sgm_dropout: y = x * keep / (1 - p), keep drawn from (seed[0], element index) by a counter-based hash; seed is a
 *   device int64.  The backward is the same call on the gradient.  n a multiple of 4 (float32) / 8 (bfloat16).
 * htrvt_sgm_xent_fwd: logits float32 [2 B L][ldv]: row log-softmax over the first V columns, NLL at tgt (clamped) times
 *   mask; logits_l / logits_r (may be NULL) float32 [B][L][V] copies; lse, rowloss [2 B L] scratch kept for the backward;
 *   rowloss64 [2 B L] float64 scratch: the row losses again, from which the scalar is reduced;
 *   den[0] = 2 max(sum mask, 1), loss[0] = sum / den[0] rounded once from float64, both by a fixed-shape ordered reduction.
 * htrvt_sgm_xent_bwd: dlogits [2 B L][ldv] (dtype) = (softmax - onehot) * mask * g[0] / den[0] (+ dlogits_l / _r, may be
 *   NULL; g may be NULL = 0), zero in the columns V .. ldv-1.
 * htrvt_sgm_convert: dst = src (accumulate: dst += src), element types src_dtype / dst_dtype. */
int htrvt_sgm_context(const int32_t* table, int B, int Lmax, int S, int pad_id, int bos_left_id, int bos_right_id, int eos_id,
                      int64_t* left, int64_t* right, int64_t* tgt, float* mask, void* stream);
int htrvt_sgm_query_fwd(const int64_t* left, const int64_t* right, const float* emb, const float* dir_left,
                        const float* dir_right, void* out, int B, int L, int S, int V, int d_txt, int dtype, void* stream);
int64_t htrvt_sgm_query_bwd_workspace_floats(int B, int L, int V, int d_txt);
int htrvt_sgm_query_bwd(const int64_t* left, const int64_t* right, const void* dq, float* workspace, float* demb,
                        float* ddir_left, float* ddir_right, int B, int L, int S, int V, int d_txt, int dtype, void* stream);
int htrvt_sgm_dropout(const void* x, void* y, int64_t n, const int64_t* seed, float p, int dtype, void* stream);
int htrvt_sgm_xent_fwd(const float* logits, int ldv, int V, int B, int L, const int64_t* tgt, const float* mask,
                       float* logits_l, float* logits_r, float* lse, float* rowloss, double* rowloss64, float* loss, float* den,
                       void* stream);
int htrvt_sgm_xent_bwd(const float* logits, int ldv, int V, int B, int L, const int64_t* tgt, const float* mask,
                       const float* lse, const float* den, const float* g, const float* dlogits_l, const float* dlogits_r,
                       void* dlogits, int dtype, void* stream);
int htrvt_sgm_convert(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, int accumulate, void* stream);

/* ---- the LGP fork's block operators (csrc/lgp.hip; model_lgp/model/plg.py) -------------------------------------------------
 * float32 and bfloat16, no float atomics (bitwise reproducible), nothing allocated, scalars read from device memory.
 * Activation and gradient tensors are accessed as 16-byte vectors: their base pointers (an offset one included, e.g. the
 * right half of a [B N][2D] buffer) must be 16-byte aligned and are refused otherwise.
 * htrvt_attn_local_*: WindowMHSA1D between its two Linear layers: softmax(q k^T scale) v inside non-overlapping windows of
 *   `window` tokens (1 ... 16), qkv [B N][3][heads][hd] as the qkv GEMM leaves it, out [B N][heads][hd], hd 64 or 128.  A
 *   window slot at token index >= N (N % window != 0: the last window of every image) is the row the Linear makes of the
 *   reference's zero padding token, k = v = qkv_bias (float32 [3 heads hd], its k and v thirds, rounded to dtype): real
 *   queries attend to it, it is NOT masked.  Nothing is saved for the backward, which recomputes the window's softmax.
 *   _bwd: dqkv [B N][3][heads][hd] written whole; dpad float32 [B][2][heads hd] overwritten with the summed gradient of each
 *   image's padding rows' k and v (zeros when N % window == 0) -- a column sum over B adds it to d qkv.bias[D : 3D].
 *   _supported: 1 if (hd, window, dtype) is served, else 0 with the reason in htrvt_last_error().
 * htrvt_attn_local_shift_*: the same kernels and argument contract with the Swin-style `shift` of WindowMHSA1D (0 <= shift <
 *   window, refused otherwise; shift 0 is bitwise htrvt_attn_local_*): the reference rolls the tokens by `shift` before it
 *   pads and rolls the cropped output back.  Here that is index arithmetic on the same [B N] buffers: token j sits in rolled
 *   slot p = (j + shift) mod N, window t holds slots [t window, (t + 1) window), slots p >= N of the last window are the
 *   padding rows (k = v = qkv_bias), and slot p < N reads qkv and writes out / dqkv at token (p - shift) mod N.  So window 0
 *   mixes the last `shift` tokens of the line with its first window - shift (no mask across the wrap), and the ragged window
 *   holds tokens N - shift - N % window ... N - shift - 1.  dpad as above.
 * htrvt_lgp_pool_norm_fwd: z [B G][D] = LayerNorm without affine (eps) of adaptive_avg_pool1d(x [B N][D]) along the tokens,
 *   bin g = tokens [floor(g N / G), ceil((g + 1) N / G)); mean / rstd float32 [B G].  1 <= G <= N, D <= 2048.
 *   _bwd: dx [B N][D] = (accumulate: +=) the gradient of x for dz, each token gathering from the bins that contain it;
 *   workspace 2 B G floats.
 * htrvt_lgp_upsample_fwd: out[b][t][0:D] (row stride ldo elements) = sigmoid(logit_alpha[0]) * linear interpolation of
 *   y [B G][D] to N tokens, F.interpolate(mode="linear", align_corners=False).
 *   _bwd: dy [B G][D] overwritten by gather from dout (row stride ldd); dlogit_alpha[0] += its gradient by a two-stage
 *   ordered sum over htrvt_lgp_upsample_bwd_workspace_floats(B, G) floats of workspace. */
int htrvt_attn_local_supported(int hd, int window, int dtype);
int htrvt_attn_local_fwd(const void* qkv, const float* qkv_bias, void* out, int B, int N, int heads, int hd, int window,
                         float scale, int dtype, void* stream);
int htrvt_attn_local_bwd(const void* qkv, const float* qkv_bias, const void* dout, void* dqkv, float* dpad, int B, int N,
                         int heads, int hd, int window, float scale, int dtype, void* stream);
int htrvt_attn_local_shift_supported(int hd, int window, int shift, int dtype);
int htrvt_attn_local_shift_fwd(const void* qkv, const float* qkv_bias, void* out, int B, int N, int heads, int hd, int window,
                               int shift, float scale, int dtype, void* stream);
int htrvt_attn_local_shift_bwd(const void* qkv, const float* qkv_bias, const void* dout, void* dqkv, float* dpad, int B, int N,
                               int heads, int hd, int window, int shift, float scale, int dtype, void* stream);
int htrvt_lgp_pool_norm_fwd(const void* x, void* z, float* mean, float* rstd, int B, int N, int G, int D, float eps, int dtype,
                            void* stream);
int htrvt_lgp_pool_norm_bwd(const void* dz, const void* z, const float* rstd, float* workspace, void* dx, int B, int N, int G,
                            int D, int accumulate, int dtype, void* stream);
int htrvt_lgp_upsample_fwd(const void* y, const float* logit_alpha, void* out, int64_t ldo, int B, int N, int G, int D,
                           int dtype, void* stream);
int64_t htrvt_lgp_upsample_bwd_workspace_floats(int B, int G);
int htrvt_lgp_upsample_bwd(const void* dout, int64_t ldd, const void* y, const float* logit_alpha, void* dy,
                           float* dlogit_alpha, float* workspace, int B, int N, int G, int D, int dtype, void* stream);

/* ---- convolutional token mixer (model_sgm_macaron/model/HTR_VT.py:148-180, ConvLocalMixer1D) between its Linear layers:
 * GLU -> depthwise Conv1d(k, padding k/2) along the tokens -> BatchNorm1d -> SiLU (csrc/mixer.hip).
 * Layout: token rows as the GEMMs leave them, no transpose.  u [B*N][2D] (the pw_in output: value half, gate half),
 * c / s / ds [B*N][D], du [B*N][2D], all of type dtype (float32 or bfloat16); w float32 [D][k] (dwconv.weight [D][1][k]);
 * per-channel vectors (scale, shift, mean, rstd, coef) float32.  g = u[:, :D] * sigmoid(u[:, D:]) and
 *   c[b][n][d] = sum_j w[d][j] * g[b][n + j - k/2][d],
 * where a term whose token index leaves 0 .. N-1 of ITS OWN image b is zero (zero padding per image: no row of another
 * image is read).  z = c * scale + shift, s = z * sigmoid(z); scale == NULL stands for 1 and shift == NULL for 0, so
 * use_bn=False is scale = NULL, shift = dwconv.bias.  c is stored rounded to dtype, and z and the statistics are taken
 * from the stored values.
 * Refused (negative return, htrvt_last_error(), nothing launched): k even or outside 1 ... 15, D not a multiple of 8,
 * u / c / s / ds / du not 16-byte aligned, B * N < 2 in htrvt_mixer_fwd_train.
 * Workspaces (float32), all reductions being per-workgroup partial rows plus an ordered second stage (no float atomics):
 *   htrvt_mixer_rows(B, N, D, dtype)                 partial rows R that fwd_train and bwd write for this shape
 *   htrvt_mixer_fwd_workspace_floats(B, N, D, dtype) (R + 64) * 2 * D: partial [R][2][D] = (sum c, sum c^2) of fwd_train,
 *       with the 64 scratch rows behind it that htrvt_bn_finalize(partial, R, D, count = B * N, ...) may use
 *   htrvt_mixer_bwd_workspace_floats(B, N, D, k, dtype)  R * D * (k + 1): dw_partial [R][D * k] (+ db_partial [R][D])
 *   htrvt_mixer_reduce_rows(rows, D, dtype)          partial rows Q of bwd_reduce: partial [Q][2][D]
 * Forward, train: htrvt_mixer_fwd_train (c, partial) -> htrvt_bn_finalize -> htrvt_mixer_bn_silu (s).
 * Forward, eval / no BatchNorm: htrvt_mixer_fwd_eval, one launch, coefficients from htrvt_bn_eval_coeffs; c may be NULL
 *   when no backward follows.
 * Backward: htrvt_mixer_bwd_reduce -> partial [Q][2][D] = (sum dz, sum dz * (c - mean) * rstd), dz = ds * silu'(z), for
 *   htrvt_bn_bwd_finalize (mean == NULL: the second sum is zero); then htrvt_mixer_bwd: dc = coef[0] * dz + coef[1] * c +
 *   coef[2] (coef [3][D] of htrvt_bn_bwd_finalize; NULL: dc = dz), dg = dc convolved with the flipped taps, du through the
 *   GLU recomputed from u; dw_partial rows sum (htrvt_colsum over D * k columns) to d w [D][k], db_partial (may be NULL)
 *   rows to d bias [D] = sum dc. */
int htrvt_mixer_rows(int B, int N, int D, int dtype);
int64_t htrvt_mixer_fwd_workspace_floats(int B, int N, int D, int dtype);
int64_t htrvt_mixer_bwd_workspace_floats(int B, int N, int D, int k, int dtype);
int htrvt_mixer_reduce_rows(int64_t rows, int D, int dtype);
int htrvt_mixer_fwd_train(const void* u, const float* w, void* c, float* partial, int B, int N, int D, int k, int dtype,
                          void* stream);
int htrvt_mixer_bn_silu(const void* c, const float* scale, const float* shift, void* s, int64_t rows, int D, int dtype,
                        void* stream);
int htrvt_mixer_fwd_eval(const void* u, const float* w, const float* scale, const float* shift, void* c, void* s, int B,
                         int N, int D, int k, int dtype, void* stream);
int htrvt_mixer_bwd_reduce(const void* ds, const void* c, const float* scale, const float* shift, const float* mean,
                           const float* rstd, float* partial, int64_t rows, int D, int dtype, void* stream);
int htrvt_mixer_bwd(const void* u, const void* c, const void* ds, const float* w, const float* scale, const float* shift,
                    const float* coef, void* du, float* dw_partial, float* db_partial, int B, int N, int D, int k, int dtype,
                    void* stream);

/* ---- the convolutional forks' blocks (model_sgm_mms_conv/model/HTR_VT.py:103-166 FeedForward and ConvModule;
 * model_sgm_mms_conv_squeeze/model/HTR_VT.py:169-223 SqueezeExcite1D, Downsample1D, Upsample1D): csrc/gnmixer.hip.
 * Token rows as the GEMMs leave them; activations of type dtype (float32 or bfloat16), 16-byte aligned, their channel count a
 * multiple of the 16-byte vector (8 bfloat16, 4 float32); statistics, parameters and parameter gradients float32; offsets
 * 64-bit.  Every sum is formed in a fixed order (no float atomics): two runs give the same bits.  Refused (negative return,
 * htrvt_last_error(), nothing launched): another dtype, a channel count off the vector, misaligned buffers, k even or outside
 * 1 ... 15, a shape whose grid does not fit one launch.
 *
 * GroupNorm mixer, ConvModule between its two 1x1 convolutions: u [B*N][2C] (pointwise_conv1's output: value half, gate half)
 *   g = u[:, :C] * sigmoid(u[:, C:]),  c[b][n][d] = bias[d] + sum_j w[d][j] * g[b][n + j - k/2][d]  (zero padding per image),
 *   z = (c - mean_b) * rstd_b * gamma + beta,  s = z * sigmoid(z),
 * mean_b and rstd_b = 1 / sqrt(var_b + eps) over ALL C * N values of image b (nn.GroupNorm(1, C), biased variance), taken
 * from c as stored (rounded to dtype).  Train and eval are the same computation.  w float32 [C][k], bias / gamma / beta [C]
 * (NULL: 0 / 1 / 0).  A workgroup's runs all lie in one image, so every partial belongs to one image:
 *   htrvt_gnmixer_rows(B, N, C, dtype)   R: workgroup rows of the launches (rows of the per-channel and dw / db partials)
 *   htrvt_gnmixer_parts(B, N, C, dtype)  P: partial pairs per image; pairs is float32 [B][P][2]
 * Forward: htrvt_gnmixer_fwd (c, pairs = (sum c, sum c^2)) -> htrvt_gn_finalize(pairs, B, P, count = C * N, eps) (mean [B],
 *   rstd [B]; the pairs added in order in float64) -> htrvt_gnmixer_act (s; also the backward's way back to s).
 * Backward, dz = ds * silu'(z), xhat = (c - mean_b) * rstd_b:
 *   htrvt_gnmixer_bwd_reduce -> chan_partial [R][2][C] = (sum dz, sum dz * xhat) per channel, whose column sums (htrvt_colsum
 *     over 2 C columns) are (d beta | d gamma), and pairs [B][P][2] = (sum gamma dz, sum gamma dz xhat) per image;
 *   htrvt_gn_bwd_finalize(pairs, B, P, count = C * N) -> m1 [B], m2 [B], the two means;
 *   htrvt_gnmixer_bwd: dc = rstd_b * (gamma dz - m1_b - xhat * m2_b) on the fly, dg = dc convolved with the flipped taps, du
 *     [B*N][2C] through the GLU recomputed from u; dw_partial [R][C * k] and db_partial [R][C] (db = sum dc), summed by
 *     htrvt_colsum. */
int htrvt_gnmixer_rows(int B, int N, int C, int dtype);
int htrvt_gnmixer_parts(int B, int N, int C, int dtype);
int htrvt_gnmixer_fwd(const void* u, const float* w, const float* bias, void* c, float* pairs, int B, int N, int C, int k,
                      int dtype, void* stream);
int htrvt_gn_finalize(const float* pairs, int B, int P, double count, float eps, float* mean, float* rstd, void* stream);
int htrvt_gnmixer_act(const void* c, const float* mean, const float* rstd, const float* gamma, const float* beta, void* s,
                      int B, int N, int C, int dtype, void* stream);
int htrvt_gnmixer_bwd_reduce(const void* ds, const void* c, const float* mean, const float* rstd, const float* gamma,
                             const float* beta, float* chan_partial, float* pairs, int B, int N, int C, int dtype,
                             void* stream);
int htrvt_gn_bwd_finalize(const float* pairs, int B, int P, double count, float* m1, float* m2, void* stream);
int htrvt_gnmixer_bwd(const void* u, const void* c, const void* ds, const float* w, const float* mean, const float* rstd,
                      const float* gamma, const float* beta, const float* m1, const float* m2, void* du, float* dw_partial,
                      float* db_partial, int B, int N, int C, int k, int dtype, void* stream);
/* Squeeze-excite gate on x [B*N][D]: y = x * g[b], g = sigmoid(fc2(silu(fc1(mean over the tokens)))), all of the MLP float32.
 * Forward: htrvt_se_mean (mean [B][D]) -> htrvt_se_mlp_fwd (one workgroup per image; fc1 w1 [H][D], b1 [H], fc2 w2 [D][H],
 *   b2 [D]; pre [B][H] = fc1's output, act = silu(pre), g [B][D]) -> htrvt_se_scale_fwd (y).
 * Backward: htrvt_se_scale_bwd_reduce (dg[b][d] = sum_n dy * x) -> htrvt_se_mlp_bwd (dh2 [B][D], dh1 [B][H]: the gradients at
 *   fc2's and fc1's outputs; dmean [B][D]) -> htrvt_se_wgrad twice (dW [M][K] = sum_b dy[b][m] x[b][k], db [M] = sum_b dy[b][m],
 *   b in increasing order: (dh2, act) for fc2, (dh1, mean) for fc1) -> htrvt_se_scale_bwd (dx = dy * g[b] + dmean[b] / N). */
int htrvt_se_mean(const void* x, float* mean, int B, int N, int D, int dtype, void* stream);
int htrvt_se_mlp_fwd(const float* mean, const float* w1, const float* b1, const float* w2, const float* b2, float* pre,
                     float* act, float* g, int B, int D, int H, void* stream);
int htrvt_se_scale_fwd(const void* x, const float* g, void* y, int B, int N, int D, int dtype, void* stream);
int htrvt_se_scale_bwd_reduce(const void* dy, const void* x, float* dg, int B, int N, int D, int dtype, void* stream);
int htrvt_se_mlp_bwd(const float* dg, const float* g, const float* pre, const float* w1, const float* w2, float* dh2, float* dh1,
                     float* dmean, int B, int D, int H, void* stream);
int htrvt_se_wgrad(const float* dy, const float* x, float* dw, float* db, int B, int M, int K, void* stream);
int htrvt_se_scale_bwd(const void* dy, const float* g, const float* dmean, void* dx, int B, int N, int D, int dtype,
                       void* stream);
/* Resampling of token rows.  down2: y[b][j] = (x[b][2j] + x[b][2j+1]) / 2, j < N / 2 (avg_pool1d(2, 2): an odd last token is
 * dropped and gets a zero gradient); N >= 2 (N <= 1 is the identity, the caller's).  up_add: out[b][i] = y[b][(i * n) / N0] +
 * skip[b][i], i < N0, 1 <= n <= N0: nearest up-sampling (F.interpolate's index) fused with the skip add; its backward sums the
 * targets of each source token in increasing order, and the skip's gradient is dout itself. */
int htrvt_seq_down2_fwd(const void* x, void* y, int B, int N, int D, int dtype, void* stream);
int htrvt_seq_down2_bwd(const void* dy, void* dx, int B, int N, int D, int dtype, void* stream);
int htrvt_seq_up_add_fwd(const void* y, const void* skip, void* out, int B, int n, int N0, int D, int dtype, void* stream);
int htrvt_seq_up_add_bwd(const void* dout, void* dy, int B, int n, int N0, int D, int dtype, void* stream);
/* FeedForward's activation between its two GEMMs (htrvt_gemm's epilogues are GELU only): a = silu(pre), dpre = da * silu'(pre),
 * n elements, a multiple of the vector */
int htrvt_silu_fwd(const void* pre, void* a, int64_t n, int dtype, void* stream);
int htrvt_silu_bwd(const void* da, const void* pre, void* dpre, int64_t n, int dtype, void* stream);

/* The VAN forks' height reducer and horizontal mixer (model_sgm_mms_attach_van/model/HTR_VT.py:159-254 LargeKernelAttention,
 * VANBlock, VANHeightReducer, HorizontalMixer; model_sgm_mms_attach_van_2 is identical): what they need beside the 1x1
 * convolutions (htrvt_gemm on the [B*H*W][C] rows) and the BatchNorm passes (htrvt_bn_*), csrc/van.hip.
 * Tensors are NHWC [B][H][W][C] of type dtype (float32 or bfloat16), C a multiple of 8, 16-byte aligned; per-channel vectors
 * and all weights are float32; sums are formed in float32 and a result is rounded once.  Depthwise weights are as torch
 * stores them, w [C][kh * kw] (Conv2d.weight [C][1][kh][kw], groups = C), no re-layout.
 *
 * Depthwise convolution, kh in {1,3,5,7}, kw in {1,3,5,7,9}, dil in 1 ... 3 (the forks: 5x5 d1, 7x7 d3, 1x9 d1):
 *   y[b][h][w][c] = sum_{i,j} w[c][i * kw + j] * x[b][h + (i - kh/2) * dil][w + (j - kw/2) * dil][c],
 * a term whose row leaves 0 .. H-1 or whose column leaves 0 .. W-1 of ITS OWN image being zero (zero padding per image: no
 * pixel of another image and nothing outside the buffer is read).  A kernel row i whose input row lies outside the image
 * for output row h is skipped as a whole -- no loads, no multiply-adds -- by a test that is uniform over the workgroup;
 * with H = 4 and dil = 3 at most 2 of 7 kernel rows are live.
 *   htrvt_van_dw_fwd         y from x.
 *   htrvt_van_dw_bwd_input   dx[b][h][w][c] = sum_{i,j} w[c][i * kw + j] * dy[b][h - (i - kh/2) * dil][w - (j - kw/2) * dil][c]
 *                            (+ add[b][h][w][c] where add != NULL: a gradient that reaches x by another path): dy convolved
 *                            with the flipped taps, same dilation, same skip of dead rows.
 *   htrvt_van_dw_bwd_weight  partial [R][C * kh * kw] float32, R = htrvt_van_dw_rows(...): the rows sum (htrvt_colsum over
 *                            C * kh * kw columns) to d w[c][i * kw + j] = sum_{b,h,w} dy[b][h][w][c] * x[b][h + (i - kh/2) *
 *                            dil][w + (j - kw/2) * dil][c]; every element of every row is written.
 *   htrvt_van_dw_bwd_workspace_floats  R * C * kh * kw.
 * Passes over rows = B * H * W pixels, [rows][C]; scale == NULL stands for 1, shift == NULL for 0:
 *   htrvt_van_moments        partial [Q][2][C] = (sum x, sum x^2) of the stored values, Q = htrvt_van_moments_rows(rows, C,
 *                            dtype) <= 128, for htrvt_bn_finalize(partial, Q, C, count = rows, ...).
 *   htrvt_van_gate_fwd       LKA gate g = a * (p * scale + shift): a the block's GELU output (the fork's u), p the pw
 *                            convolution's output, scale / shift its BatchNorm's (htrvt_bn_finalize or htrvt_bn_eval_coeffs).
 *   htrvt_van_gate_bwd       from dg: da = dg * (p * scale + shift), the part of d a through the gate's first factor, and
 *                            dz = dg * a, the gradient of the BatchNorm output, laid out as htrvt_bn_bwd_reduce and
 *                            htrvt_bn_bwd_apply take it.
 *   htrvt_van_bn_res_gelu_fwd  y = gelu(res + x * scale + shift), exact (erf) GELU; res == NULL: without the shortcut.
 *   htrvt_van_bn_res_gelu_bwd  dt = dy * gelu'(res + x * scale + shift), recomputed from x, scale, shift, res: the gradient
 *                            of the shortcut and of the BatchNorm output.
 * Height pool: htrvt_van_hpool_fwd  y[b][w][c] = mean_h x[b][h][w][c]; htrvt_van_hpool_bwd  dx[b][h][w][c] = d[b][w][c] / H.
 * Every reduction is per-workgroup partial rows plus an ordered second stage (no float atomics): the gradients are bitwise
 * reproducible.  Refused (negative return, htrvt_last_error(), nothing launched): kh / kw even or outside the set, dil outside
 * 1 ... 3, C not a multiple of 8, a tensor that is not 16-byte aligned, a null required pointer, B * H > 65535. */
int htrvt_van_dw_fwd(const void* x, const float* w, void* y, int B, int H, int W, int C, int kh, int kw, int dil, int dtype,
                     void* stream);
int htrvt_van_dw_bwd_input(const void* dy, const float* w, const void* add, void* dx, int B, int H, int W, int C, int kh,
                           int kw, int dil, int dtype, void* stream);
int htrvt_van_dw_rows(int B, int H, int W, int C, int kh, int kw, int dil, int dtype);
int64_t htrvt_van_dw_bwd_workspace_floats(int B, int H, int W, int C, int kh, int kw, int dil, int dtype);
int htrvt_van_dw_bwd_weight(const void* x, const void* dy, float* partial, int B, int H, int W, int C, int kh, int kw, int dil,
                            int dtype, void* stream);
int htrvt_van_moments_rows(int64_t rows, int C, int dtype);
int htrvt_van_moments(const void* x, float* partial, int64_t rows, int C, int dtype, void* stream);
int htrvt_van_gate_fwd(const void* a, const void* p, const float* scale, const float* shift, void* g, int64_t rows, int C,
                       int dtype, void* stream);
int htrvt_van_gate_bwd(const void* dg, const void* a, const void* p, const float* scale, const float* shift, void* da,
                       void* dz, int64_t rows, int C, int dtype, void* stream);
int htrvt_van_bn_res_gelu_fwd(const void* x, const float* scale, const float* shift, const void* res, void* y, int64_t rows,
                              int C, int dtype, void* stream);
int htrvt_van_bn_res_gelu_bwd(const void* dy, const void* x, const float* scale, const float* shift, const void* res, void* dt,
                              int64_t rows, int C, int dtype, void* stream);
int htrvt_van_hpool_fwd(const void* x, void* y, int B, int H, int W, int C, int dtype, void* stream);
int htrvt_van_hpool_bwd(const void* d, void* dx, int B, int H, int W, int C, int dtype, void* stream);

/* ---- Swin fork (csrc/swin.hip): WindowAttention2D inside SwinBlock2D of model_sgm_mms_swin/model/HTR_VT.py, between the
 * qkv and proj Linear layers: attention in 2-D windows of wh x ww <= 32 tokens of an H x W token map, with the learned
 * relative-position bias, the 2-D cyclic shift and the fork's additive mask across the wrap.
 *   qkv [B H W][3][heads][hd] in plain token order (b, h, w), as the qkv GEMM leaves it; out [B H W][heads][hd] and dqkv in
 *   that same order; table float32 [(2wh-1)(2ww-1)][heads], the parameter as stored.  Roll, window partition, window reverse
 *   and roll-back are index arithmetic: window (i, j), i < H / wh, j < W / ww, slot t = r ww + c sits at the shifted
 *   coordinate (hs, ws) = (i wh + r, j ww + c) and reads qkv / writes out and dqkv at token ((hs + sh) mod H, (ws + sw) mod W)
 *   -- torch.roll(x, (-sh, -sw)) before the partition and roll(.., (sh, sw)) after the merge.
 *   S[t][u] = scale q_t.k_u + table[(r_t - r_u + wh - 1)(2ww - 1) + (c_t - c_u + ww - 1)][head] + m(t, u), softmax over u,
 *   out_t = sum_u P[t][u] v_u.  m is SwinBlock2D._build_attn_mask: the region of a slot is the pair (sh > 0 and hs >= H - sh,
 *   sw > 0 and ws >= W - sw) -- TWO regions per shifted axis, not standard Swin's three -- and m = -100.0 where the regions
 *   of t and u differ, else 0.  The mask is ADDED: a masked pair whose raw score lies more than 100 above the rest still wins.
 *   _bwd saves nothing but qkv: it recomputes the window's softmax, writes dqkv whole, and writes the table gradient as
 *   partial rows, dtable_partial float32 [htrvt_attn_win2d_rows(..)][(2wh-1)(2ww-1) heads]: row p is the ordered sum of
 *   dS[t][u] (the gradient of the pre-softmax score, without `scale`) into the table entry of (t, u) over the p-th share of
 *   the B (H / wh)(W / ww) (image, window) items.  The rows (at most 256) are added by htrvt_rowsum_f32, htrvt_colsum's ordered
 *   second stage (htrvt_colsum itself takes columns in fours; the fork's table has 630 entries).  No float atomics: two runs
 *   give the same bits.
 *   Served: float32 and bfloat16, hd 32 / 64 / 128, wh, ww >= 1 with wh ww <= 32, H % wh == 0, W % ww == 0, 0 <= sh < wh,
 *   0 <= sw < ww, base pointers 16-byte aligned.  Everything else: a non-zero return, the reason in htrvt_last_error(),
 *   nothing launched.  _supported: 1 if (hd, wh, ww, dtype) is served, else 0 with the reason set.  _rows: -1 if refused. */
int htrvt_attn_win2d_supported(int hd, int wh, int ww, int dtype);
int htrvt_attn_win2d_fwd(const void* qkv, const float* table, void* out, int B, int H, int W, int heads, int hd, int wh, int ww,
                         int sh, int sw, float scale, int dtype, void* stream);
int htrvt_attn_win2d_rows(int B, int H, int W, int heads, int wh, int ww);
int htrvt_attn_win2d_bwd(const void* qkv, const float* table, const void* dout, void* dqkv, float* dtable_partial, int B, int H,
                         int W, int heads, int hd, int wh, int ww, int sh, int sw, float scale, int dtype, void* stream);

/* ---- SVTR fork (csrc/svtr.hip): MultiHeadSelfAttention(local=True) of model_sgm_mms_svtr/model/svtr.py, between the qkv and
 * proj Linear layers: 2-D neighbourhood attention.  Query (h, w) of the H x W token map attends to the keys (h', w') of the
 * map with |h - h'| <= kh / 2 and |w - w'| <= kw / 2 (integer halves) -- the fork's dense scores plus its -inf mask, where a
 * masked key has weight exactly 0.  Keys outside the map do not exist: they are never read and contribute nothing.
 *   qkv [B H W][3][heads][hd] in plain token order (b, h, w), as the (bias-free) qkv GEMM leaves it; out, dout [B H W][heads][hd];
 *   dqkv as qkv.  lse float32 [B heads][H W]: log sum_k exp(scale q.k) over the query's keys; NULL in a forward-only call.
 *   out = sum_k softmax_k(scale q.k) v_k.
 *   _bwd recomputes P = exp(scale q.k - lse) from qkv and lse, forms delta = dO . out itself (no workspace) and writes dqkv
 *   whole, in two launches of one kernel: dq over each query's box, then dk / dv over each key's box (the box is symmetric,
 *   so the queries that see a key are the key's own box).  No float atomics: two runs give the same bits.
 *   Served: float32 and bfloat16, hd 32 / 64, kh and kw odd with 1 <= kh <= 7, 1 <= kw <= 11, any H, W >= 1 (H < kh and
 *   W < kw included), any B >= 0 and heads >= 1, base pointers 16-byte aligned.  Offsets are 64-bit, so the operands may pass
 *   2 GiB; the bound is the grid: B heads ceil(H / 4) ceil(W / 16) workgroups must stay below 2^31.  Everything else: a
 *   non-zero return, the reason in htrvt_last_error(), nothing launched.  _supported: 1 if (hd, kh, kw, dtype) is served,
 *   else 0 with the reason set. */
int htrvt_attn_nbr2d_supported(int hd, int kh, int kw, int dtype);
int htrvt_attn_nbr2d_fwd(const void* qkv, void* out, float* lse, int B, int H, int W, int heads, int hd, int kh, int kw,
                         float scale, int dtype, void* stream);
int htrvt_attn_nbr2d_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int B, int H, int W,
                         int heads, int hd, int kh, int kw, float scale, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HTRVT_H */
