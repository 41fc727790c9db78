// valid.hip -- the metric half of model_v1/valid.py:49-75 on the device: per sample the Levenshtein distance between the
// greedy-decoded prediction and the label, once over characters (editdistance.eval(pred, gt), valid.py:50) and once over the
// word lists of utils.format_string_for_wer(...).split(" ") (valid.py:59-63, utils/utils.py:176-179).
//
// One workgroup of two waves per sample.  Both sequences are staged in LDS as canonical symbol indices, cut into word spans
// there (a scan over the symbol kinds), and every word gets an id: the first target word it equals symbol for symbol, or
// "none".  Then wave 0 runs the character table and wave 1 the word table at the same time.  Each is an anti-diagonal
// wavefront with the lanes along the target: lane l owns the K columns l*K+1 .. l*K+K in registers, works on row s - l + 1
// in step s, and takes the cell to its left from lane l - 1 by DPP; the diagonal cell is what it took one step earlier.
// Nothing proportional to len(pred) x len(target) exists anywhere.
#include "common.h"

namespace htrvt {
namespace {

constexpr int EC_NT = 128;          // wave 0: characters, wave 1: words; both stage and tokenise
constexpr int EC_KMAX = 8;          // columns per lane
constexpr int EC_MAX_TGT = 64 * EC_KMAX;
constexpr int EC_MAX_PRED = 16384;  // htrvt_ctc_greedy_decode's T limit
constexpr int EC_NONE = 0xffff;     // id of a prediction word that equals no target word

typedef unsigned short u16;

// lane l <- lane l - 1 (DPP wave_shr:1); lane 0 <- first
__device__ __forceinline__ int lane_from_left(int first, int v) { return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xf, 0xf, false); }

__device__ __forceinline__ bool is_ordinary(int k) { return k == 0 || k == 3; }

// Word spans of a sequence with the symbol kinds k[0:L) by the rule of format_string_for_wer + split(" "): white space (kinds 1, 3) at both ends goes
// (str.strip), then every punctuation symbol (2) is a word, every maximal run of ordinary symbols (0, and 3 inside the
// string) is a word and separators (1) only divide.  No word at all = one empty word.  All EC_NT threads; returns the count.
__device__ int word_spans(const unsigned char* k, int L, u16* ws, u16* we, int* scratch) {
  const int tid = threadIdx.x;
  int* lohi = scratch + EC_NT;
  if (tid == 0) {
    lohi[0] = L;
    lohi[1] = 0;
  }
  __syncthreads();
  int lo = L, hi = 0;
  for (int i = tid; i < L; i += EC_NT)
    if (k[i] != 1 && k[i] != 3) {
      lo = min(lo, i);
      hi = i + 1;
    }
  if (lo < L) {
    atomicMin(&lohi[0], lo);
    atomicMax(&lohi[1], hi);
  }
  __syncthreads();
  lo = lohi[0];
  hi = max(lohi[1], lo);
  const int per = (hi - lo + EC_NT - 1) / EC_NT;
  const int i0 = min(hi, lo + tid * per), i1 = min(hi, i0 + per);
  int ns = 0, ne = 0;
  for (int i = i0; i < i1; ++i) {
    const int c = k[i];
    const bool o = is_ordinary(c);
    ns += (c == 2 || (o && (i == lo || !is_ordinary(k[i - 1])))) ? 1 : 0;
    ne += (c == 2 || (o && (i == hi - 1 || !is_ordinary(k[i + 1])))) ? 1 : 0;
  }
  scratch[tid] = ns | (ne << 16);   // both at most 16384
  __syncthreads();
  int s0 = 0, e0 = 0, total = 0;
  for (int t = 0; t < EC_NT; ++t) {
    const int v = scratch[t];
    if (t < tid) {
      s0 += v & 0xffff;
      e0 += v >> 16;
    }
    total += v & 0xffff;
  }
  for (int i = i0; i < i1; ++i) {
    const int c = k[i];
    const bool o = is_ordinary(c);
    if (c == 2 || (o && (i == lo || !is_ordinary(k[i - 1])))) ws[s0++] = (u16)i;
    if (c == 2 || (o && (i == hi - 1 || !is_ordinary(k[i + 1])))) we[e0++] = (u16)(i + 1);
  }
  if (total == 0 && tid == 0) ws[0] = we[0] = 0;
  __syncthreads();
  return max(total, 1);
}

__device__ __forceinline__ bool same_symbols(const int* a, const int* b, int n) {
  for (int i = 0; i < n; ++i)
    if (a[i] != b[i]) return false;
  return true;
}

// Levenshtein distance (unit costs) of a[0:La) against the Lb <= 64 K symbols spread over the lanes, b[k] = column
// lane * K + k.  One wave.  a is read 64 rows at a time into a register and handed down the lanes with the wavefront.
template <int K, class TA>
__device__ int wave_levenshtein(const TA* a, int La, const int (&b)[K], int Lb, int lane) {
  int cur[K];   // row i - 1 of the lane's columns; row 0 is 1, 2, 3, ...
#pragma unroll
  for (int k = 0; k < K; ++k) cur[k] = lane * K + k + 1;
  int diag = lane * K;   // D[i-1][lane * K]
  int av = 0, abuf = 0;
  const int steps = La + max(1, (Lb + K - 1) / K) - 1;
  for (int s = 0; s < steps; ++s) {
    if ((s & 63) == 0) abuf = s + lane < La ? (int)a[s + lane] : 0;
    av = lane_from_left(__builtin_amdgcn_readlane(abuf, s & 63), av);   // a[s - lane]
    const int i = s - lane + 1;
    int left = lane_from_left(i, cur[K - 1]);                           // D[i][lane * K]
    if (i >= 1 && i <= La) {
      int lf = left, dg = diag;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int up = cur[k];
        const int v = min(min(up, lf) + 1, dg + (av != b[k] ? 1 : 0));
        dg = up;
        lf = v;
        cur[k] = v;
      }
      diag = left;
    }
  }
  if (Lb == 0) return La;
  int v = cur[0];
#pragma unroll
  for (int k = 1; k < K; ++k) v = ((Lb - 1) % K == k) ? cur[k] : v;
  return __shfl(v, (Lb - 1) / K, 64);
}

template <int K>
__global__ __launch_bounds__(EC_NT) void error_counts_kernel(const int* __restrict__ pred, long long ld_pred,
                                                             const int* __restrict__ pred_len, const int* __restrict__ tgt,
                                                             const int* __restrict__ tgt_len, const int* __restrict__ tgt_off,
                                                             const int* __restrict__ canon, const unsigned char* __restrict__ kind,
                                                             int nsym, int max_pred, int max_tgt, int np, int* __restrict__ counts,
                                                             unsigned long long* __restrict__ totals) {
  constexpr int TW = 64 * K;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  int* pc = reinterpret_cast<int*>(smem_raw);         // [np] prediction, canonical
  int* tc = pc + np;                                  // [TW] target, canonical
  int* scratch = tc + TW;                             // [EC_NT + 2]
  u16* ps = reinterpret_cast<u16*>(scratch + EC_NT + 2);   // [np] prediction word starts, then their ids
  u16* pe = ps + np;                                  // [np] ... ends (exclusive)
  u16* ts = pe + np;                                  // [TW] target word starts
  u16* te = ts + TW;                                  // [TW] ... ends
  u16* tw = te + TW;                                  // [TW] ... ids
  unsigned char* pk = reinterpret_cast<unsigned char*>(tw + TW);   // [np] kinds of the prediction
  unsigned char* tk = pk + np;                        // [TW] kinds of the target

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Lp = min(max(pred_len[b], 0), max_pred), Lt = min(max(tgt_len[b], 0), max_tgt);
  const int* pr = pred + (long long)b * ld_pred;
  const int* tr = tgt + tgt_off[b];
  // an index outside the tables stands for itself and is an ordinary symbol
  for (int i = tid; i < Lp; i += EC_NT) {
    const int r = pr[i];
    const bool in = (unsigned)r < (unsigned)nsym;
    pc[i] = in ? canon[r] : r;
    pk[i] = in && kind[r] <= 3 ? kind[r] : 0;
  }
  for (int i = tid; i < Lt; i += EC_NT) {
    const int r = tr[i];
    const bool in = (unsigned)r < (unsigned)nsym;
    tc[i] = in ? canon[r] : r;
    tk[i] = in && kind[r] <= 3 ? kind[r] : 0;
  }
  __syncthreads();
  const int Wp = word_spans(pk, Lp, ps, pe, scratch);
  const int Wt = word_spans(tk, Lt, ts, te, scratch);
  // target word j: the first target word with the same symbols (itself if there is none before it)
  for (int j = tid; j < Wt; j += EC_NT) {
    const int s = ts[j], n = te[j] - s;
    int id = j;
    for (int j2 = 0; j2 < j; ++j2)
      if (te[j2] - ts[j2] == n && same_symbols(tc + ts[j2], tc + s, n)) {
        id = j2;
        break;
      }
    tw[j] = (u16)id;
  }
  __syncthreads();
  // prediction word i: the id of the target words it equals; written over its start, which only this thread reads
  for (int i = tid; i < Wp; i += EC_NT) {
    const int s = ps[i], n = pe[i] - s;
    int id = EC_NONE;
    for (int j = 0; j < Wt; ++j)
      if (tw[j] == j && te[j] - ts[j] == n && same_symbols(tc + ts[j], pc + s, n)) {
        id = j;
        break;
      }
    ps[i] = (u16)id;
  }
  __syncthreads();

  int sym[K];
  int dist, len;
  if (wave == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) sym[k] = lane * K + k < Lt ? tc[lane * K + k] : 0;
    dist = wave_levenshtein<K>(pc, Lp, sym, Lt, lane);
    len = Lt;
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k) sym[k] = lane * K + k < Wt ? (int)tw[lane * K + k] : 0;
    dist = wave_levenshtein<K>(ps, Wp, sym, Wt, lane);
    len = Wt;
  }
  if (lane == 0) {
    counts[b * 4 + wave * 2] = dist;
    counts[b * 4 + wave * 2 + 1] = len;
    if (totals) {
      atomicAdd(totals + wave * 2, (unsigned long long)dist);
      atomicAdd(totals + wave * 2 + 1, (unsigned long long)len);
    }
  }
}

size_t lds_bytes(int K, int np) { return (size_t)np * 9 + (size_t)64 * K * 11 + (EC_NT + 2) * 4; }

template <int K>
int launch(const int32_t* pred, int64_t ld_pred, const int32_t* pred_len, const int32_t* tgt, const int32_t* tgt_len,
           const int32_t* tgt_off, const int32_t* canon, const uint8_t* kind, int nsym, int B, int max_pred, int max_tgt,
           int32_t* counts, int64_t* totals, hipStream_t st) {
  const int np = ((max_pred > 0 ? max_pred : 1) + 3) / 4 * 4;   // keeps every array 4-byte aligned
  const size_t smem = lds_bytes(K, np);
  if (smem > 64 * 1024 && allow_dynamic_lds<error_counts_kernel<K>>((int)lds_bytes(K, EC_MAX_PRED), "htrvt_error_counts")) return -2;
  hipLaunchKernelGGL(error_counts_kernel<K>, dim3(B), dim3(EC_NT), smem, st, pred, (long long)ld_pred, pred_len, tgt, tgt_len,
                     tgt_off, canon, kind, nsym, max_pred, max_tgt, np, counts, reinterpret_cast<unsigned long long*>(totals));
  set_last_kernel("error_counts_kernel<%d>", K);
  return check_launch("error_counts");
}

}  // namespace
}  // namespace htrvt

using namespace htrvt;

extern "C" int htrvt_error_counts_max_tgt(void) { return EC_MAX_TGT; }

extern "C" int htrvt_error_counts(const int32_t* pred, int64_t ld_pred, const int32_t* pred_len, const int32_t* tgt,
                                  const int32_t* tgt_len, const int32_t* tgt_off, const int32_t* canon, const uint8_t* kind,
                                  int nsym, int B, int max_pred, int max_tgt, int32_t* counts, int64_t* totals, void* stream) {
  HTRVT_REQUIRE(pred && pred_len && tgt && tgt_len && tgt_off && canon && kind && counts,
                "htrvt_error_counts: null pointer (only totals may be null)");
  HTRVT_REQUIRE(B > 0 && nsym > 0, "htrvt_error_counts: B=%d and nsym=%d must be positive", B, nsym);
  HTRVT_REQUIRE(max_pred >= 0 && max_pred <= EC_MAX_PRED, "htrvt_error_counts: max_pred=%d outside [0, %d] (the greedy decode's limit)",
                max_pred, EC_MAX_PRED);
  HTRVT_REQUIRE(max_tgt >= 0 && max_tgt <= EC_MAX_TGT,
                "htrvt_error_counts: max_tgt=%d outside [0, %d] (htrvt_error_counts_max_tgt)", max_tgt, EC_MAX_TGT);
  HTRVT_REQUIRE(ld_pred >= max_pred, "htrvt_error_counts: ld_pred=%lld < max_pred=%d", (long long)ld_pred, max_pred);
  hipStream_t st = (hipStream_t)stream;
#define EC_LAUNCH(K) launch<K>(pred, ld_pred, pred_len, tgt, tgt_len, tgt_off, canon, kind, nsym, B, max_pred, max_tgt, counts, totals, st)
  if (max_tgt <= 64) return EC_LAUNCH(1);
  if (max_tgt <= 128) return EC_LAUNCH(2);
  if (max_tgt <= 256) return EC_LAUNCH(4);
  return EC_LAUNCH(8);
#undef EC_LAUNCH
}
