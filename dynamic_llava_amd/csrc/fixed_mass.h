// The fixed-point token mass shared by the device sampler (sample.hip) and the device scorer (score.hip): sampling.py S_BITS / MAX_VOCAB.
#pragma once
#include "dl_common.h"

namespace dl {

constexpr int kSampleMassBits = 40;  // sampling.py S_BITS
constexpr int kSampleMaxV = 65536;   // V * 2^40 < 2^63

// floor(w * 2^40) for 0 <= w <= 1 (exact: a shift of the significand)
__device__ __forceinline__ uint64_t sample_mass(float w) {
  const uint32_t u = __float_as_uint(w);
  const int e = (int)((u >> 23) & 255u);
  if (e == 0 || e > 127 || (u >> 31)) return 0;  // zero / denormal (< 2^-126) / negative / not a weight (> 1, inf, NaN)
  const uint64_t mant = (uint64_t)((u & 0x7fffffu) | 0x800000u);
  const int sh = e - 127 - 23 + kSampleMassBits;
  return sh >= 0 ? (mant << sh) : (sh > -24 ? (mant >> (-sh)) : 0ull);
}

}  // namespace dl
