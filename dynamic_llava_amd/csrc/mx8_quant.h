// The MXFP8 quantisation rule of dynamic_llava_amd/mxfp8.py for one block of 32 elements, as device helpers (the statements of
// quantize_mx8_kernel in gemv_mx8.hip): amax == 0 -> e = 0 and every code 0; else e = clamp(floor(log2(amax)) - 8, e_min, 127) and
// code = RNE(v / 2^e) to e4m3fn, saturated at +-448.  Used where a block is spread over several lanes (the KV-cache kernels).
#pragma once
#include "dl_common.h"

namespace dl {

// block exponent of a block whose largest magnitude is amax (finite, >= 0)
__device__ __forceinline__ int mx8_block_exp(float amax, int e_min) {
  if (!(amax > 0.f)) return 0;
  const uint32_t ab = __float_as_uint(amax);
  const int ex = (int)(ab >> 23);
  const int fl = ex != 0 ? ex - 127 : (31 - __clz((int)(ab & 0x7fffffu))) - 149;  // floor(log2(amax)), fp32 subnormals included
  const int e = fl - 8;
  return e < e_min ? e_min : (e > 127 ? 127 : e);
}

// 2^-e as two fp32 factors (e in [-124, 127]): both stay normal (2^-127 alone is not)
__device__ __forceinline__ void mx8_inv_scale(int e, float& inv_hi, float& inv_lo) {
  inv_hi = __uint_as_float((uint32_t)(127 - (e >> 1)) << 23);
  inv_lo = __uint_as_float((uint32_t)(127 - (e - (e >> 1))) << 23);
}

// e4m3fn code of v / 2^e (block amax > 0)
__device__ __forceinline__ uint32_t mx8_code(float v, float inv_hi, float inv_lo) {
  const float s = (v * inv_hi) * inv_lo;  // exact unless it underflows fp32 (then it rounds to 0 in e4m3 either way)
  const float a = fabsf(s);
  const uint32_t sign = __float_as_uint(s) >> 31;
  // quantum of a in e4m3: 2^(floor(log2 a) - 3) for a >= 2^-6, 2^-9 below
  const int ea = (int)((__float_as_uint(a) >> 23) & 0xffu) - 127;
  const int qe = ea >= -6 ? ea - 3 : -9;
  const float quantum = __uint_as_float((uint32_t)(qe + 127) << 23);
  float r = rintf(a / quantum) * quantum;  // RNE (a / quantum is exact: a power of two)
  r = fminf(r, 448.0f);
  const uint32_t rb = __float_as_uint(r);
  const int er = (int)(rb >> 23) - 127;
  uint32_t mag;
  if (r == 0.f) mag = 0u;
  else if (er >= -6) mag = ((uint32_t)(er + 7) << 3) | ((rb >> 20) & 7u);
  else mag = (uint32_t)(r * 512.0f);  // subnormal: multiples of 2^-9
  return (sign << 7) | mag;
}

// E8M0 code -> 2^(code - 127) as fp32 (codes 1..254; the quantiser writes 3..254)
__device__ __forceinline__ float mx8_pow2(uint32_t code) { return __uint_as_float(code << 23); }

}  // namespace dl
