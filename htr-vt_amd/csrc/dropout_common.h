// dropout_common.h -- the counter-based dropout mask, defined once: htrvt_sgm_dropout (sgm.hip), the residual / drop-path
// op (dropout.hip) and the attention kernels that regenerate the mask on chip (attention_impl.h) all draw from here.
//
//   keep(seed, i) = top 24 bits of mix64(seed + G * (i + 1)) >= thr,   thr = (unsigned)(p * 2^24 + 0.5)
// a pure function of the seed (an int64 read from the device) and the element's logical index i, never of the thread that
// evaluates it.  The hash input is linear in i modulo 2^64, so a kernel may form `seed + G * (i + 1)` once per row and step
// it by multiples of G (hash_input / keep_hashed); keep_elem is the same expression from the index.
#pragma once

#include "common.h"

namespace htrvt {

constexpr unsigned long long DROP_G = 0x9e3779b97f4a7c15ull;      // the golden-ratio step of splitmix64

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {   // splitmix64 finaliser
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ unsigned long long hash_input(unsigned long long seed, unsigned long long i) {
  return seed + DROP_G * (i + 1);
}
__device__ __forceinline__ bool keep_hashed(unsigned long long z, unsigned thr) {
  return (unsigned)(mix64(z) >> 40) >= thr;   // 24 uniform bits: P(keep) = 1 - thr / 2^24
}
__device__ __forceinline__ bool keep_elem(unsigned long long seed, long long i, unsigned thr) {
  return keep_hashed(hash_input(seed, (unsigned long long)i), thr);
}

// host side: what a probability p in [0, 1) becomes in the kernels
struct DropRate {
  unsigned thr;      // an element is dropped when its 24 bits are below thr
  float scale;       // 1 / (1 - p) on the kept ones
};
inline DropRate drop_rate(float p) {
  return DropRate{(unsigned)((double)p * 16777216.0 + 0.5), (float)(1.0 / (1.0 - (double)p))};
}

}  // namespace htrvt
