// gemm_halo_impl.h -- 3x3, stride-1, pad-1 convolution forward / dgrad as implicit GEMM with a HALO-STAGED A operand
// (resnet18.py:26-31: nine of the twelve 3x3 convolutions of the stem, forward and input gradient).
//
// The generic gather kernel (gemm_dma_impl.h, GATHER 1 / 2) stages, for each of the nine taps and each 64-channel
// chunk, its own 256 x 64 A tile: the pixels of the three taps of one kernel row are the same pixels shifted by one
// column, so two thirds of the A bytes that cross the (per-CU, ~50-70 GB/s) LDS-DMA path are re-reads -- and that path,
// not the matrix pipe, bounds the k-tile (2 450 cycles per k-tile against 1 536 for the MFMAs).
// Here an M tile is 256 consecutive pixels of ONE image row (host check: W % 256 == 0); per (kernel row, channel chunk)
// ONE halo tile of 258 pixels x 64 channels is staged and serves three k-tiles, the MFMA waves reading their A
// fragments `shift` rows further down for the next tap.  Operand bytes per three k-tiles: 40 KB (33 real) + 3 x 24 KB
// instead of 3 x 56 KB.  The freed LDS pays for a third B stage: B runs two k-tiles ahead, the halo tile a whole group
// ahead, and every wait is a counted vmcnt that leaves the newest k-tile's pieces in flight.
//
// Structure otherwise as gemm_dma_kernel<256, BN, .., SPEC = 1>: 8 MFMA waves (4 x 2, v_mfma_f32_16x16x32_bf16: halo_ktile)
// + 4 loader waves, one barrier per k-tile, the LDS-staged bf16 epilogue (BatchNorm column sums; backward-of-ReLU mask and
// BatchNorm-backward sums on dgrad) shared with that kernel.
//
// Three kernels run on ONE skeleton (below the epilogue helpers: halo_tile, halo_roles, HaloLoader, halo_kernarg,
// halo_launch): gemm_halo_kernel (stride 1, and the forward with a row stride), gemm_halo_fs2_kernel (forward with a column
// stride of 2: odd / even pixel images) and gemm_halo_s2_kernel (strided dgrad, all parity classes in one launch).  Each body
// holds its geometry, its consumer k-tile walk and its loader schedule with the counted waits -- what differs -- and nothing
// else.
#pragma once
#include "gemm_dma_impl.h"

namespace {

template <int BN>
struct HaloGeo {
  static constexpr int BM = 256;
  static constexpr int A_PIECES = 40;                    // 320 LDS rows of 128 B: rows 0..257 are pixels w0-1 .. w0+256, the rest zero fill
  static constexpr int A_STAGE = A_PIECES * 1024;
  static constexpr int B_STAGE = Geo<BN>::BYTES;
  static constexpr int NP_B = B_STAGE / 1024 / 4;        // B pieces per loader wave and k-tile
  static constexpr int NP_AH = A_PIECES / 2 / 4;         // A pieces per loader wave in each of a group's first two k-tiles
  static constexpr unsigned B_BASE = 2 * A_STAGE;
  static constexpr int LDS_BYTES = 2 * A_STAGE + 3 * B_STAGE;
  static_assert(B_STAGE % 4096 == 0, "B pieces divide over the four loader waves");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS");
};


// One k-tile (64 deep) of a consumer wave: its 64 x (32 TN) block from a halo A stage (fragments read `shift` rows down)
// and a K-major B stage, then the k-tile's barrier.  v_mfma_f32_16x16x32_bf16: 4 x (2 TN) tiles of 16 x 16, two k-steps
// of 32.  Operand lane map: row l & 15, 16-byte k chunk 4 s + (l >> 4).  Measured against the v_mfma_f32_32x32x16_bf16 form of the same loop (same bytes from LDS, same
// cycles per FLOP): +2.4 ... +6 % on every stride-1 3x3 convolution of the stem, forward and dgrad
// (profiles/r05_experiments.md) -- the chip holds a higher clock on this shape (MI355X_MICROARCH.md, DVFS give-back,
// item 7).
typedef float f32x4h_t __attribute__((ext_vector_type(4)));
template <int BN>
__device__ __forceinline__ void halo_ktile(f32x4h_t (&a4)[4][BN / 32], const char* sa, const char* sb, int shift, int wm, int wn, int lane) {
  constexpr int TM = 2, TN = BN / 64;
  const int arow16 = wm * 64 + (lane & 15), ag = lane >> 4;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    bf16x8_t fa[2 * TM], fb[2 * TN];
    const int chunk = 4 * s + ag;
#pragma unroll
    for (int i = 0; i < 2 * TM; ++i) {
      const int row = arow16 + i * 16 + shift;
      fa[i] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(sa + row * 128 + ((chunk ^ Geo<256>::swz(row)) << 4)));
    }
#pragma unroll
    for (int j = 0; j < 2 * TN; ++j) {
      const int row = wn * TN * 32 + j * 16 + (lane & 15);
      fb[j] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(sb + row * 128 + ((chunk ^ Geo<BN>::swz(row)) << 4)));
    }
#pragma unroll
    for (int i = 0; i < 2 * TM; ++i)
#pragma unroll
      for (int j = 0; j < 2 * TN; ++j)
        a4[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], a4[i][j], 0, 0, 0);
  }
  __builtin_amdgcn_s_barrier();
}
// the four 16 x 16 tiles of 32 x 32 block (i, j) as registers 4 (2 a + b) + r of acc[i][j] (epilogue_staged<..., MF = 16>)
template <int TM, int TN>
__device__ __forceinline__ void halo_acc16_to_32(f32x16_t (&acc)[TM][TN], const f32x4h_t (&a4)[2 * TM][2 * TN]) {
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[i][j][4 * (2 * a + b) + r] = a4[2 * i + a][2 * j + b][r];
}

// float32 C straight from the 16 x 16 accumulator tiles (the split-bf16 parity path, csrc/split.hip: its convolutions are bf16
// products over three times the channels with float32 results; until round 5 they ran on the generic gather because the halo
// kernels only had the LDS-staged bf16 epilogue).  a4[i][j][r] = C(row 16 i + 4 (lane >> 4) + r, column 16 j + (lane & 15)) of the
// wave's 64 x (32 TN) block: plain stores (16 lanes = 64 contiguous bytes of one row), alpha, an optional float32 residual (dgrad),
// and the per-tile BatchNorm column sums of the forward (wave partials through LDS, summed over the four wave rows in a fixed
// order).  Every wave of the workgroup calls it (loader waves with active = false: they only join the barrier).
template <int BN, int TM, int TN, int NTH, bool CSTATS, class P>
__device__ __forceinline__ void halo_epilogue_f32(const f32x4h_t (&a4)[2 * TM][2 * TN], const P& p, int m0, int n0, int wm, int wn,
                                                  int tile_m, int lane, char* smem, bool active) {
  float* const Cf = reinterpret_cast<float*>(p.C);
  const float* const Rf = reinterpret_cast<const float*>(p.residual);
  const int lr = lane & 15, lg = lane >> 4;
  float s1[2 * TN], s2[2 * TN];
#pragma unroll
  for (int j = 0; j < 2 * TN; ++j) s1[j] = s2[j] = 0.f;
  if (active) {
#pragma unroll
    for (int j = 0; j < 2 * TN; ++j) {
      const int n = n0 + wn * TN * 32 + 16 * j + lr;
      const bool nok = n < p.N;
#pragma unroll
      for (int i = 0; i < 2 * TM; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = m0 + wm * 64 + 16 * i + 4 * lg + r;
          const float a = a4[i][j][r];       // rows >= M and columns >= N hold exact zeros (zero-filled operands)
          if constexpr (CSTATS) {
            s1[j] += a;
            s2[j] = fmaf(a, a, s2[j]);
          }
          if (nok && m < p.M) {
            const long long o = (long long)m * p.ldc + n;
            float v = a * p.alpha;
            if (Rf != nullptr) v += Rf[o];
            Cf[o] = v;
          }
        }
      }
    }
  }
  if constexpr (CSTATS) {
    if (p.colstats != nullptr) {      // workgroup-uniform
      float* red = reinterpret_cast<float*>(smem);     // [4 wave rows][BN][2]; the operand stages are dead
#pragma unroll
      for (int j = 0; j < 2 * TN; ++j) {
        float a = s1[j], q = s2[j];
        a += __shfl_xor(a, 16, 64); q += __shfl_xor(q, 16, 64);
        a += __shfl_xor(a, 32, 64); q += __shfl_xor(q, 32, 64);
        if (lane < 16 && active) {
          const int c = wn * TN * 32 + 16 * j + lane;
          red[(wm * BN + c) * 2 + 0] = a;
          red[(wm * BN + c) * 2 + 1] = q;
        }
      }
      __syncthreads();
      for (int c = threadIdx.x; c < BN; c += NTH) {
        const int n = n0 + c;
        if (n < p.N) {
          float a = 0.f, q = 0.f;
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            a += red[(w * BN + c) * 2];
            q += red[(w * BN + c) * 2 + 1];
          }
          float* dst = p.colstats + (long long)tile_m * 2 * p.N;
          dst[n] = a;
          dst[p.N + n] = q;
        }
      }
    }
  }
}

// =============================================================================================
// The skeleton the three bodies below run on (stride-1 forward / dgrad, column-stride-2 forward, merged strided dgrad): tile
// map, wave roles with the two barriers every tile has, the loader waves' lane state with the A-piece loop, the end of a
// tile, the kernel-argument reference and the launch.  A body supplies its geometry and its two k-tile walks, nothing else.
// =============================================================================================
constexpr int HALO_NWC = 8, HALO_NW = 12;                 // 8 MFMA waves (4 x 2) + 4 loader waves = 768 threads
typedef const __attribute__((address_space(4))) KParams HaloKP;

// Block -> (tile_m, tile_n).  Workgroup b runs on XCD b % 8: with a tile count that is a multiple of 8 every XCD gets a
// CONTIGUOUS eighth of the tiles; any other count stays in grid order.  This is NOT xcd_tile_id (gemm8p_impl.h): that map also chunks counts that are no multiple of 8, and
// switching to it would move tiles between XCDs -- a change of behaviour, not of spelling.
template <class P>
__device__ __forceinline__ void halo_tile(const P& p, int block_x, int& tile_m, int& tile_n) {
  const int ntiles = p.tiles_m * p.tiles_n;
  const int id = (ntiles & 7) == 0 ? (block_x & 7) * (ntiles >> 3) + (block_x >> 3) : block_x;
  tile_m = id / p.tiles_n;
  tile_n = id - tile_m * p.tiles_n;
}

template <int NI, int NJ>
__device__ __forceinline__ void halo_zero(f32x4h_t (&a4)[NI][NJ]) {
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) a4[i][j] = f32x4h_t{0.f, 0.f, 0.f, 0.f};
}

// Lane state of a loader wave: B (the packed weights, K-major) through a DmaLoader, A as 1-KiB pieces of a pixel image.
// Piece lw + 4 i of an image holds its LDS rows 32 i + 8 lw .. + 7; this lane fills row rho0 + 32 i, 16-byte chunk cgA (the
// read swizzle applied to the SOURCE chunk: the DMA writes lane-linear).
template <int BN>
struct HaloLoader {
  DmaLoader<BN, HTRVT_KMAJOR, 0, 4> lb;
  i32x4_t rsrcA;
  int lw, rho0, cgA;
  unsigned lds0;

  template <class P>
  __device__ __forceinline__ void init(const P& p, int n0, int lw_, int lane, const char* smem) {
    lw = lw_;
    lb.init(p, p.B, p.ldb, n0, p.N, lw, lane);
    rsrcA = make_rsrc(p.A);
    rho0 = lw * 8 + (lane >> 3);
    cgA = (lane & 7) ^ Geo<256>::swz(rho0);
    lds0 = lds_addr_of(smem);
  }

  // Pieces i0 .. i0 + NP - 1 (per loader wave) of the image at LDS byte offset lds_off: LDS row r < nvalid holds channels
  // [64 chunk, 64 chunk + 64) of source pixel src0 + STEP r of the pixel row whose chunk starts at byte gbase; every other
  // row, a pixel outside [0, Ww), a channel >= Cs and everything when !rowok are zero fill (offset OOB).  32 LDS rows per
  // piece = 32 STEP source pixels.  lane_off may wrap for a negative first pixel: masked by the pixel test.
  // Plain values only: a select over by-reference captures became a run-time index into a scratch-resident closure (see
  // group_base in gemm_halo_s2_body).
  template <int NP, int STEP>
  __device__ __forceinline__ void issueA(int i0, unsigned lds_off, int nvalid, bool rowok, unsigned gbase, int chunk, int src0, int Ww,
                                         int Cs) const {
    const bool chok = rowok && chunk * BK + cgA * 8 < Cs;
    const int wl = src0 + STEP * rho0;
    const unsigned lane_off = (unsigned)(wl * Cs + cgA * 8) * 2u;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int ii = i0 + i;
      const int rho = rho0 + 32 * ii;
      const int w = wl + STEP * 32 * ii;
      const bool v = chok && rho < nvalid && (unsigned)w < (unsigned)Ww;
      const unsigned voff = v ? gbase + lane_off + (unsigned)(STEP * 32 * ii * Cs) * 2u : OOB;
      dma16(rsrcA, __builtin_amdgcn_readfirstlane(lds0 + lds_off + (lw + 4 * ii) * 1024), voff);
    }
  }

  // the B k-tile at weight column k0 -> LDS byte offset lds_off; k0 >= kend: zero fill
  template <class P>
  __device__ __forceinline__ void issueB(const P& p, unsigned lds_off, int k0, int kend) {
    lb.template issue<true>(p, lds0 + lds_off, k0, kend, lw);
  }
};

// The two roles of a tile.  Waves 0..7 are consumers, 4 x 2 as (wm, wn); waves 8..11 are loaders lw = 0..3 at priority 3.
// Between the opening and the closing barrier:
//   consume(a4, wm, wn, lane): the body's k-tile walk, one halo_ktile (MFMAs + barrier) per k-tile
//   load(L, open):             the body's prologue, open() = the counted wait that leaves only the second B k-tile in flight +
//                              the opening barrier, then the loader's walk with one barrier per k-tile, and the drain
// Consumer and loader waves run SEPARATE straight-line copies of the loop (same barriers) -- fragment reads + MFMAs between
// barriers on one side, nothing but address arithmetic and DMA issue on the other.  In one loop walked by every wave, the
// register allocation, the scalar state and the instruction stream of either role carried the other's: the split form is
// -5 ... -9 % per launch on every stride-1 3x3 convolution of the stem (profiles/r05_experiments.md).
// finish: the end of a tile -- float32 C straight from the 16 x 16 tiles, or the LDS-staged bf16 epilogue shared with
// gemm_dma_kernel (DGRAD / CSTATS: the paths it compiles in; rmul: its C row stride, sw in the merged strided dgrad).  It is
// inlined once per role and the role is a compile-time constant: the loader waves' copy (they only join the epilogue's
// barriers and walk its store phase) is compiled against constant zeros and holds no accumulators.  How the constant reaches
// the epilogue matters to hipcc: through a run-time flag, or through one more function around this one,
// gemm_halo_kernel<192, true> grows by 4 ... 9 % (the epilogue's run-time feature walk, profiles/halo_one_skeleton.md).
template <int BN, bool DGRAD, bool CSTATS, bool F32, class P, class Consume, class Load>
__device__ __forceinline__ void halo_roles(const P& p, char* smem, int m0, int n0, int tile_m, int rmul, Consume&& consume, Load&& load) {
  constexpr int TM = 2, TN = BN / 64;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = (wave >> 1) & 3, wn = wave & 1;
  auto finish = [&](const f32x4h_t (&a4)[2 * TM][2 * TN], auto active) __attribute__((always_inline)) {
    constexpr bool ACTIVE = decltype(active)::value;
    if constexpr (F32) {
      halo_epilogue_f32<BN, TM, TN, HALO_NW * 64, CSTATS>(a4, p, m0, n0, wm, wn, tile_m, lane, smem, ACTIVE);
    } else {
      f32x16_t acc[TM][TN];
      halo_acc16_to_32<TM, TN>(acc, a4);
      epilogue_staged<TN, BN, 256, HALO_NW, DGRAD, CSTATS, P, 16>(acc, p, 0ll, m0, n0, wm, wn, tile_m, lane, wave, smem, ACTIVE, rmul);
    }
  };
  f32x4h_t a4[2 * TM][2 * TN];
  if (wave < HALO_NWC) {
    halo_zero(a4);
    __builtin_amdgcn_s_barrier();
    consume(a4, wm, wn, lane);
    __builtin_amdgcn_s_barrier();
    finish(a4, std::true_type{});
  } else {
    __builtin_amdgcn_s_setprio(3);
    HaloLoader<BN> L;
    L.init(p, n0, (wave - HALO_NWC) & 3, lane, smem);
    load(L, []() __attribute__((always_inline)) {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(HaloGeo<BN>::NP_B) : "memory");
      __builtin_amdgcn_s_barrier();
    });
    __builtin_amdgcn_s_barrier();
    halo_zero(a4);
    finish(a4, std::false_type{});
  }
}

// The parameters are read where they lie, in the kernarg segment (the struct is the kernel's only argument: offset 0), through
// a constant-address-space reference: scalar loads, never a private copy of the struct.
__device__ __forceinline__ HaloKP& halo_kernarg() { return *(HaloKP*)__builtin_amdgcn_kernarg_segment_ptr(); }

// one workgroup per tile; `fmt`, ...: the symbol as htrvt_last_kernel reports it
template <auto KERN, int LDS, class... Args>
int halo_launch(const KParams& p, hipStream_t st, const char* what, const char* fmt, Args... args) {
  if (int rc = allow_dynamic_lds<KERN>(LDS, what)) return rc;
  hipLaunchKernelGGL(KERN, dim3(p.tiles_m * p.tiles_n), dim3(HALO_NW * 64), LDS, st, p);
  set_last_kernel(fmt, args...);
  const int rc = check_launch(what);
  return rc ? rc : 1;
}

// ---------------------------------------------------------------------------------------------
// Stride-1 forward / dgrad (the file header's kernel).
// DGRAD = false: A rows = output pixels, source = x [B,H,W,Ci];  true: A rows = input pixels, source = dy [B,H,W,Co].
// Forward with a row stride (sh = 2, W stride 1: the first conv of layer 1): M rows are OUTPUT rows, Hm = Ho of them per image,
// and kernel row gdy of output row h reads input row h * sh + gdy - 1; dgrad is served at stride 1 only.
// ---------------------------------------------------------------------------------------------
template <int BN, bool DGRAD, bool F32, class P>
__device__ __forceinline__ void gemm_halo_body(const P& p, const int block_x) {
  using H = HaloGeo<BN>;
  constexpr int BM = 256;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  int tile_m, tile_n;
  halo_tile(p, block_x, tile_m, tile_n);
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int Hh = DGRAD ? p.Ho : p.Hi, Ww = DGRAD ? p.Wo : p.Wi, Cs = DGRAD ? p.Co : p.Ci;   // gathered tensor [B,Hh,Ww,Cs]
  const int rowi = m0 / Ww, w0 = m0 - rowi * Ww;
  const int Hm = DGRAD ? Hh : p.Ho;                     // forward with a row stride: M rows are OUTPUT rows
  const int bimg = rowi / Hm, hrow = rowi - bimg * Hm;
  const int NC = p.Cpad / BK;
  // Kernel rows that read the image: row gdy of this tile reads source row hh(gdy), the same for all 256 pixels, and a row in
  // the padding (the top / bottom image row; both at H = 1) would be NC groups of MFMAs over a zero-filled halo tile -- exact
  // +0 terms.  The valid rows are the contiguous range [glo, ghi], which always holds 1; BOTH roles walk exactly these
  // (ghi - glo + 1) * NC groups, so their barrier counts agree for every range.
  const int hh0 = DGRAD ? hrow + 1 : hrow * p.sh - 1, hh2 = DGRAD ? hrow - 1 : hrow * p.sh + 1;   // hh(0), hh(2)
  const int glo = __builtin_amdgcn_readfirstlane((unsigned)hh0 < (unsigned)Hh ? 0 : 1);
  const int ghi = __builtin_amdgcn_readfirstlane((unsigned)hh2 < (unsigned)Hh ? 2 : 1);
  const int NG = (ghi - glo + 1) * NC;

  halo_roles<BN, DGRAD, !DGRAD, F32>(
      p, smem, m0, n0, tile_m, 1,
      [&](auto& a4, int wm, int wn, int lane) __attribute__((always_inline)) {
        for (int g = 0; g < NG; ++g) {
          const char* sa = smem + (g & 1) * H::A_STAGE;
          halo_ktile<BN>(a4, sa, smem + H::B_BASE + 0 * H::B_STAGE, DGRAD ? 2 : 0, wm, wn, lane);
          halo_ktile<BN>(a4, sa, smem + H::B_BASE + 1 * H::B_STAGE, 1, wm, wn, lane);
          halo_ktile<BN>(a4, sa, smem + H::B_BASE + 2 * H::B_STAGE, DGRAD ? 0 : 2, wm, wn, lane);
        }
      },
      [&](HaloLoader<BN>& L, auto open) __attribute__((always_inline)) {
        // half `half` of the halo tile of group (gdy, gcc) -> A stage `ast`
        auto issueA = [&](int half, int ast, int gdy, int gcc) {
          const int hh = DGRAD ? hrow + 1 - gdy : hrow * p.sh + gdy - 1;
          const unsigned gbase = (unsigned)(((bimg * Hh + hh) * Ww) * Cs + gcc * BK) * 2u;
          L.template issueA<H::NP_AH, 1>(half * H::NP_AH, ast * H::A_STAGE, 258, (unsigned)hh < (unsigned)Hh, gbase, gcc, w0 - 1, Ww, Cs);
        };
        auto issueB = [&](int bst, int gdy, int gcc, int dx) {
          L.issueB(p, H::B_BASE + bst * H::B_STAGE, (gdy * 3 + dx) * p.Cpad + gcc * BK, p.K);
        };
        // ---- prologue: halo tile of group 0 = (glo, chunk 0), B of k-tiles 0 and 1 ----
        issueA(0, 0, glo, 0);
        issueA(1, 0, glo, 0);
        issueB(0, glo, 0, 0);
        issueB(1, glo, 0, 1);
        open();
        int gdy = glo, gcc = 0;                  // the B offsets keep the true kernel row: (gdy * 3 + dx) * Cpad
        for (int g = 0; g < NG - 1; ++g) {       // every group but the last, (ghi, NC - 1)
          int ndy = gdy, ncc = gcc + 1;
          if (ncc == NC) {
            ncc = 0;
            ++ndy;
          }
          const int nast = (g + 1) & 1;
          issueB(2, gdy, gcc, 2);
          issueA(0, nast, ndy, ncc);
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(H::NP_B + H::NP_AH) : "memory");
          __builtin_amdgcn_s_barrier();
          issueB(0, ndy, ncc, 0);
          issueA(1, nast, ndy, ncc);
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(H::NP_B + H::NP_AH) : "memory");
          __builtin_amdgcn_s_barrier();
          issueB(1, ndy, ncc, 1);
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(H::NP_B) : "memory");
          __builtin_amdgcn_s_barrier();
          gdy = ndy;
          gcc = ncc;
        }
        // ---- last group: its third B tile, nothing left to stage for a next group ----
        issueB(2, gdy, gcc, 2);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(H::NP_B) : "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_s_barrier();
      });
}

template <int BN, bool DGRAD, bool F32 = false>
__global__ __launch_bounds__(768) void gemm_halo_kernel(const KParams p) {
  (void)p;
  gemm_halo_body<BN, DGRAD, F32>(halo_kernarg(), (int)blockIdx.x);
}

template <int BN, bool DGRAD, bool F32 = false>
int launch_halo(const KParams& p, hipStream_t st) {
  return halo_launch<gemm_halo_kernel<BN, DGRAD, F32>, HaloGeo<BN>::LDS_BYTES>(
      p, st, "gemm_halo_kernel", F32 ? "gemm_halo_kernel<%d, %s, f32>" : "gemm_halo_kernel<%d, %s>", BN, DGRAD ? "true" : "false");
}

// ---------------------------------------------------------------------------------------------
// 3x3 pad-1 convolution FORWARD with a COLUMN stride of 2 on halo-staged tiles (resnet18.py:26: conv1 of layer2.0 / layer3.0,
// stride (2,2); round 5 -- these launches ran on the generic per-row gather until now).
//
// Output pixel (ho, wo) reads x(ho sh + dy - 1, 2 wo + dx - 1).  An M tile is 256 consecutive output pixels wo0 .. wo0 + 255 of
// one output row: its column taps dx = 0 and dx = 2 read the ODD input pixels 2 wo0 - 1, 2 wo0 + 1, ... (dx = 2 the same
// pixels as dx = 0, one tile row further down) and dx = 1 the EVEN pixels 2 wo0, 2 wo0 + 2, ...  Per (kernel row, 64-channel
// chunk) = "unit": ONE odd image of 257 pixels serves two k-tiles (row shift 0 / 1) and one even image of 256 pixels the third
// -- 36 + 32 DMA pieces instead of 3 x 32, and the loader waves form one address per piece instead of decoding a pixel per
// row and tap.  k-tile order inside a unit: dx = 0, dx = 2 (odd image, LDS stage X), dx = 1 (even image, stage Y).  B runs
// two k-tiles ahead through three stages as in gemm_halo_body; the even image of a unit is issued during the unit's first
// k-tile and has two k-tiles to land; the odd image of the NEXT unit can only be issued when the current unit's second
// k-tile has read stage X for the last time, i.e. during the third k-tile, and must land within it (a second odd stage
// would need 170 KB with three B stages).
// ---------------------------------------------------------------------------------------------
template <int BN>
struct HaloFs2Geo {
  static constexpr int NPO = 9, NPE = 8;                  // 1-KiB pieces per loader wave: odd image (288 rows, 257 used), even image (256 rows)
  static constexpr int X_BYTES = 4 * NPO * 1024, Y_BYTES = 4 * NPE * 1024;
  static constexpr int B_STAGE = Geo<BN>::BYTES;
  static constexpr int NP_B = B_STAGE / 1024 / 4;
  static constexpr unsigned Y_BASE = X_BYTES, B_BASE = X_BYTES + Y_BYTES;
  static constexpr int LDS_BYTES = X_BYTES + Y_BYTES + 3 * B_STAGE;
  static_assert(B_STAGE % 4096 == 0 && LDS_BYTES <= 160 * 1024, "LDS");
  static_assert(LDS_BYTES >= BN * Stg<256>::CST, "the staged epilogue's column-major image");
  static_assert(NP_B == HaloGeo<BN>::NP_B, "halo_roles waits on the B pieces of one k-tile");
};

template <int BN, bool F32, class P>
__device__ __forceinline__ void gemm_halo_fs2_body(const P& p, const int block_x) {
  using H = HaloFs2Geo<BN>;
  constexpr int BM = 256;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  int tile_m, tile_n;
  halo_tile(p, block_x, tile_m, tile_n);
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int rowo = m0 / p.Wo, wo0 = m0 - rowo * p.Wo;     // output row (b * Ho + ho), first output column of this tile
  const int bimg = rowo / p.Ho, ho = rowo - bimg * p.Ho;
  const int NC = p.Cpad / BK;
  // kernel rows that read the image, [ulo, uhi] (always holds 1), as in gemm_halo_body: a row in the padding would be NC units
  // of exact +0 terms; both roles walk the same (uhi - ulo + 1) * NC units
  const int ulo = __builtin_amdgcn_readfirstlane((unsigned)(ho * p.sh - 1) < (unsigned)p.Hi ? 0 : 1);
  const int uhi = __builtin_amdgcn_readfirstlane((unsigned)(ho * p.sh + 1) < (unsigned)p.Hi ? 2 : 1);
  const int NU = (uhi - ulo + 1) * NC;                    // units = (kernel row, chunk); k-tiles = 3 NU

  halo_roles<BN, false, true, F32>(
      p, smem, m0, n0, tile_m, 1,
      [&](auto& a4, int wm, int wn, int lane) __attribute__((always_inline)) {
        for (int u = 0; u < NU; ++u) {
          halo_ktile<BN>(a4, smem, smem + H::B_BASE + 0 * H::B_STAGE, 0, wm, wn, lane);               // dx = 0
          halo_ktile<BN>(a4, smem, smem + H::B_BASE + 1 * H::B_STAGE, 1, wm, wn, lane);               // dx = 2
          halo_ktile<BN>(a4, smem + H::Y_BASE, smem + H::B_BASE + 2 * H::B_STAGE, 0, wm, wn, lane);   // dx = 1
        }
      },
      [&](HaloLoader<BN>& L, auto open) __attribute__((always_inline)) {
        const int Hh = p.Hi, Ww = p.Wi, Cs = p.Ci;
        // image `par` (0 odd -> stage X: source pixels 2 wo0 - 1 + 2 r, 1 even -> stage Y: 2 wo0 + 2 r) of unit (udy, ucc);
        // uvalid false: zero fill
        auto issueA = [&](int par, int udy, int ucc, bool uvalid) {
          const int hh = ho * p.sh + udy - 1;
          const bool rowok = uvalid && (unsigned)hh < (unsigned)Hh;
          const unsigned gbase = (unsigned)(((bimg * Hh + hh) * Ww) * Cs + ucc * BK) * 2u;
          if (par == 0) L.template issueA<H::NPO, 2>(0, 0, 257, rowok, gbase, ucc, 2 * wo0 - 1, Ww, Cs);
          else L.template issueA<H::NPE, 2>(0, H::Y_BASE, 256, rowok, gbase, ucc, 2 * wo0, Ww, Cs);
        };
        auto issueB = [&](int bst, int udy, int ucc, int dx, bool uvalid) {
          L.issueB(p, H::B_BASE + bst * H::B_STAGE, uvalid ? (udy * 3 + dx) * p.Cpad + ucc * BK : p.K, p.K);
        };
        // ---- prologue: odd image of unit 0 = (ulo, chunk 0), B of k-tiles 0 (dx = 0) and 1 (dx = 2) ----
        issueA(0, ulo, 0, true);
        issueB(0, ulo, 0, 0, true);
        issueB(1, ulo, 0, 2, true);
        open();
        int udy = ulo, ucc = 0;
        for (int u = 0; u < NU; ++u) {
          int ndy = udy, ncc = ucc + 1;
          if (ncc == NC) {
            ncc = 0;
            ++ndy;
          }
          const bool nvalid = u + 1 < NU;
          // k-tile 3u (dx = 0): B of this unit's third k-tile; its even image (two k-tiles to land)
          issueB(2, udy, ucc, 1, true);
          issueA(1, udy, ucc, true);
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(H::NP_B + H::NPE) : "memory");
          __builtin_amdgcn_s_barrier();
          // k-tile 3u + 1 (dx = 2): B of the next unit's first k-tile; the even image has landed behind this wait
          issueB(0, ndy, ncc, 0, nvalid);
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(H::NP_B) : "memory");
          __builtin_amdgcn_s_barrier();
          // k-tile 3u + 2 (dx = 1): stage X is free -- the next unit's odd image, then B of its second k-tile
          issueA(0, ndy, ncc, nvalid);
          issueB(1, ndy, ncc, 2, nvalid);
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(H::NP_B) : "memory");
          __builtin_amdgcn_s_barrier();
          udy = ndy;
          ucc = ncc;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the zero-fill pieces issued past the last k-tile
      });
}

template <int BN, bool F32 = false>
__global__ __launch_bounds__(768) void gemm_halo_fs2_kernel(const KParams p) {
  (void)p;
  gemm_halo_fs2_body<BN, F32>(halo_kernarg(), (int)blockIdx.x);
}

template <int BN, bool F32 = false>
int launch_halo_fs2(const KParams& p, hipStream_t st) {
  return halo_launch<gemm_halo_fs2_kernel<BN, F32>, HaloFs2Geo<BN>::LDS_BYTES>(
      p, st, "gemm_halo_fs2_kernel", F32 ? "gemm_halo_fs2_kernel<%d, f32>" : "gemm_halo_fs2_kernel<%d>", BN);
}

// ---------------------------------------------------------------------------------------------
// Strided 3x3 pad-1 convolution, INPUT GRADIENT, all stride-parity classes in ONE launch on halo-staged tiles
// (resnet18.py:26,59-63: conv1 of each stage's first block, stride (2,1) / (2,2), and its 1x1 downsample branch).
//
// dx[hi][wi] receives the taps (dy, dx) with (hi + 1 - dy) % 2 == 0 and (wi + 1 - dx) % sw == 0, i.e. a pixel of
// parity class (a, b) = (hi & 1, wi % sw) contracts a fixed tap subset against dY pixels at FIXED offsets from its
// coarse position (hq, wq) = (hi >> 1, wi / sw):
//     a = 0: kernel row 1 <- dY row hq          a = 1: kernel row 0 <- dY row hq + 1, kernel row 2 <- dY row hq
//     sw = 1:        kernel columns 0, 1, 2 <- dY columns wq + 1, wq, wq - 1
//     sw = 2, b = 0: kernel column 1 <- wq      b = 1: kernel column 0 <- wq + 1, kernel column 2 <- wq
// An M tile is 256 consecutive coarse pixels of one coarse row and ONE class: per (kernel row, 64-channel chunk) ONE
// halo tile of dY (coarse pixels wq0 - 1 .. wq0 + 256) serves the class's 1-3 column taps, exactly as in the stride-1
// kernel above -- the per-class launches of the generic gather kernel staged one 256 x 64 A tile per tap, every class
// launch re-read dY, and the class rows were scattered by a per-row index remap.  Tiles of the classes of one coarse
// row are neighbours in the grid (same XCD: dY rows are read once), the heavier classes first.
// A2 (HtrvtGemmDesc.A2): the gradient of the block's 1x1 downsample conv output rides along as three more single-tap
// groups of the class-(0, 0) tiles (source = A + extra_off, weight slot 9), as in the per-class form.
// Groups have 1, 2 or 3 k-tiles; the next group's halo tile is issued during the current group's first k-tile(s) and
// always BEFORE the B pieces of the group's last k-tile, so the counted wait of that k-tile covers it.
// ---------------------------------------------------------------------------------------------
template <int BN, class P>
__device__ __forceinline__ void gemm_halo_s2_body(const P& p, const int block_x) {
  using H = HaloGeo<BN>;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  int tile_m, tile_n;
  halo_tile(p, block_x, tile_m, tile_n);
  const int n0 = tile_n * BN;
  // tile_m -> (coarse row, class, segment): classes of one coarse row are neighbours, heaviest first
  const int sw = p.sw, ncls = 2 * sw;
  const int segs = p.Wq >> 8;                               // 256-pixel segments per coarse row (host: Wq % 256 == 0)
  const int per_row = ncls * segs;
  const int rowq = tile_m / per_row, rem = tile_m - rowq * per_row;
  const int cidx = rem / segs, seg = rem - cidx * segs;
  const int ca = 1 - cidx / sw;                             // row parity of this tile's pixels
  const int cb = sw == 2 ? 1 - (cidx & 1) : 0;              // column parity (sw = 2)
  const int bimg = rowq / p.Hq, hq = rowq - bimg * p.Hq;
  const int wq0 = seg << 8;
  const int Hh = p.Ho, Ww = p.Wo, Cs = p.Co;                // gathered tensor dY [B, Ho, Wo, Co]: Ho = Hq, Wo = Wq
  // kernel rows / columns of this class, 2 bits per entry (wave-uniform scalars).  Row parity 1 in the LAST coarse row: kernel
  // row 0 would read dY row Hq, i.e. the padding (NC groups of exact +0 terms, the first ones of the tile) -- such a tile has
  // the single row slot (kernel row 2 <- dY row hq); everything below, in both roles, derives from nrow / dyp / dhp
  const bool two = ca && hq + 1 < Hh;
  const int nrow = two ? 2 : 1;
  const int dyp = two ? (0 | (2 << 2)) : (ca ? 2 : 1);      // kernel row of row slot r
  const int dhp = two ? (1 | (0 << 2)) : 0;                  // dY row = hq + dh
  const int ncol = sw == 1 ? 3 : (cb ? 2 : 1);
  const int dxp = sw == 1 ? (0 | (1 << 2) | (2 << 4)) : (cb ? (0 | (2 << 2)) : 1);   // kernel column of column slot j
  const int shp = sw == 1 ? (2 | (1 << 2) | (0 << 4)) : (cb ? (2 | (1 << 2)) : 1);   // halo row shift of column slot j
  const int NC = p.Cpad / BK;
  const bool has_x = p.extra_off != 0 && ca == 0 && cb == 0;
  const int nmain = nrow * NC;                              // groups of the 3x3 taps
  const int ngroups = nmain + (has_x ? NC : 0);
  const int xtap = p.kh * p.kw;                             // weight slot of the 1x1 downsample conv
  const int kend = (xtap + 1) * p.Cpad;

  // Row slots of this tile: slot s < nrow = a kernel row of the 3x3 (dY row hq + dh), slot nrow = the 1x1 downsample
  // gradient (A2).  abase[s]: byte offset of (bimg, source row, pixel 0, channel 0) from p.A, OOB for a row outside dY.
  unsigned abase0, abase1, abasex;
  {
    const int h0 = hq + (dhp & 3), h1 = hq + ((dhp >> 2) & 3);
    abase0 = (unsigned)h0 < (unsigned)Hh ? (unsigned)(((bimg * Hh + h0) * Ww) * Cs) * 2u : OOB;
    abase1 = (nrow > 1 && (unsigned)h1 < (unsigned)Hh) ? (unsigned)(((bimg * Hh + h1) * Ww) * Cs) * 2u : OOB;
    abasex = has_x ? (unsigned)(((bimg * Hh + hq) * Ww) * Cs) * 2u + p.extra_off : OOB;
  }
  const int nslot = nrow + (has_x ? 1 : 0);
  // byte offset of (slot as, chunk ac)'s first pixel row, OOB for a row outside dY / past the last group.  (Formed HERE, on
  // plain values: inside a by-reference lambda hipcc turned the select over the three captured bases into a run-time
  // index into the closure object, which then lived in scratch memory together with the DMA descriptors.)
  auto group_base = [](int as, int ac, int nslot_, int nrow_, unsigned b0, unsigned b1, unsigned bx) -> unsigned {
    const unsigned rb = as >= nslot_ ? OOB : (as == nrow_ ? bx : (as == 0 ? b0 : b1));
    return rb < OOB ? rb + (unsigned)(ac * BK) * 2u : OOB;
  };

  // C rows: pixel (bimg, 2 hq + ca, sw (wq0 + r) + cb) of the NHWC gradient, r = 0 .. 255
  const int m0 = (bimg * p.Hi + 2 * hq + ca) * p.Wi + sw * wq0 + cb;

  halo_roles<BN, true, false, false>(
      p, smem, m0, n0, tile_m, sw,
      [&](auto& a4, int wm, int wn, int lane) __attribute__((always_inline)) {
        int bst = 0;
        for (int g = 0; g < ngroups; ++g) {
          const int n = g < nmain ? ncol : 1;
          const char* sa = smem + (g & 1) * H::A_STAGE;
          for (int j = 0; j < n; ++j) {
            const int shift = g < nmain ? (shp >> (2 * j)) & 3 : 1;
            halo_ktile<BN>(a4, sa, smem + H::B_BASE + bst * H::B_STAGE, shift, wm, wn, lane);
            bst = bst == 2 ? 0 : bst + 1;
          }
        }
      },
      [&, abase0, abase1, abasex](HaloLoader<BN>& L, auto open) __attribute__((always_inline)) {
        // the halo tile at `gbase` (chunk ac) -> A stage `ast`, half `half`; gbase = OOB: zero fill
        auto issueA = [&](int half, int ast, unsigned gbase, int ac) {
          L.template issueA<H::NP_AH, 1>(half * H::NP_AH, ast * H::A_STAGE, 258, gbase < OOB, gbase, ac, wq0 - 1, Ww, Cs);
        };
        // the k-tile sequence as the B loader walks it (two k-tiles ahead of the multiply): (slot, chunk, column slot)
        int bs = 0, bc = 0, bj = 0;
        auto issueB = [&](int bst) {
          int k0 = kend;                                          // past the last k-tile: zero fill
          if (bs < nslot) {
            const bool x = bs == nrow;
            const int tap = x ? xtap : ((dyp >> (2 * bs)) & 3) * 3 + ((dxp >> (2 * bj)) & 3);
            k0 = tap * p.Cpad + bc * BK;
            if (++bj == (x ? 1 : ncol)) {
              bj = 0;
              if (++bc == NC) {
                bc = 0;
                ++bs;
              }
            }
          }
          L.issueB(p, H::B_BASE + bst * H::B_STAGE, k0, kend);
        };
        // ---- prologue: halo tile of group 0, B of k-tiles 0 and 1 ----
        const unsigned gb0 = group_base(0, 0, nslot, nrow, abase0, abase1, abasex);
        issueA(0, 0, gb0, 0);
        issueA(1, 0, gb0, 0);
        issueB(0);
        issueB(1);
        open();
        int bst = 0;                     // B stage of the k-tile being multiplied; the loaders fill (bst + 2) % 3
        int gs = 0, gc = 0;              // (slot, chunk) of group g
        for (int g = 0; g < ngroups; ++g) {
          const int n = g < nmain ? ncol : 1;
          int ns = gs, nc = gc + 1;      // group g + 1
          if (nc == NC) {
            nc = 0;
            ++ns;
          }
          const unsigned ngb = group_base(ns, nc, nslot, nrow, abase0, abase1, abasex);
          const int nast = (g + 1) & 1;
          for (int j = 0; j < n; ++j) {
            const bool last = j == n - 1;
            const int fill = bst >= 1 ? bst - 1 : 2;          // (bst + 2) % 3
            if (n == 1) {             // both halves of the next halo tile, then B: the wait below covers the halo tile
              issueA(0, nast, ngb, nc);
              issueA(1, nast, ngb, nc);
              issueB(fill);
              asm volatile("s_waitcnt vmcnt(%0)" ::"n"(H::NP_B) : "memory");
            } else if (n == 2) {      // k-tile 0: B + both halves (they have the group's second k-tile to land); k-tile 1: B
              issueB(fill);
              if (j == 0) {
                issueA(0, nast, ngb, nc);
                issueA(1, nast, ngb, nc);
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(H::NP_B + 2 * H::NP_AH) : "memory");
              } else {
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(H::NP_B) : "memory");
              }
            } else {                  // three k-tiles: the schedule of the stride-1 kernel
              issueB(fill);
              if (!last) {
                issueA(j, nast, ngb, nc);
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(H::NP_B + H::NP_AH) : "memory");
              } else {
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(H::NP_B) : "memory");
              }
            }
            __builtin_amdgcn_s_barrier();
            bst = bst == 2 ? 0 : bst + 1;
          }
          gs = ns;
          gc = nc;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the zero-fill pieces issued past the last k-tile
      });
}

template <int BN>
__global__ __launch_bounds__(768) void gemm_halo_s2_kernel(const KParams p) {
  (void)p;
  gemm_halo_s2_body<BN>(halo_kernarg(), (int)blockIdx.x);
}

template <int BN>
int launch_halo_s2(const KParams& p, hipStream_t st) {
  return halo_launch<gemm_halo_s2_kernel<BN>, HaloGeo<BN>::LDS_BYTES>(p, st, "gemm_halo_s2_kernel", "gemm_halo_s2_kernel<%d>", BN);
}

}  // namespace
