// MXFP8 decoder weights (OCP Microscaling v1.0, E4M3 "e4m3fn" elements, one E8M0 scale per 32 consecutive K elements of a row):
//   dl_quantize_mx8 -- W [N,K] (f32 / bf16 / f16) -> q uint8 [N,K] + scale uint8 [N,K/32], bit-exact to dynamic_llava_amd/mxfp8.py
//   dl_gemv_mx8     -- dl_gemv's contract (PLAIN, ADDNORM, ADDNORM | OUT_SILU_PAIR; B <= dl_gemv_max_batch) on (q, scale) instead of W.
//
// The decode step at B <= 3 streams its weights and nothing else (gemv.hip): 1.06 bytes per weight instead of 2 is the whole point.
//
// Numerics.  W' = q * 2^e is exactly representable in the model dtype (the quantiser clamps e to the dtype's e_min), so the model with MXFP8 weights
// IS the model dtype's model with weights W'.  Each 16-byte chunk (16 weights, half a scale block) is converted to the activation dtype with
// v_cvt_scalef32_pk_{bf16,f16,f32}_fp8 at a unit scale (exact: every e4m3 value is a normal number of all three types), multiplied with x by
// v_dot2_f32_{bf16,f16} / fp32 FMA into a per-chunk fp32 partial p, and the block exponent is applied to p: acc = fma(p, 2^e, acc).  A power of two
// commutes with fp32 rounding, so this is the fp32 sum of the products x * W' (the exact products with W'), in a fixed order, rounded once to the
// output dtype -- dl_gemv's contract.  Applying 2^e to p and not inside the conversion keeps the dtype's subnormals out of the conversion
// instruction (fp16 blocks at e = -15 hold many of them) and costs one FMA per chunk and row instead of a scale per element.
//
// Mapping: as gemv.hip's generic kernel -- x (B rows, after the prologue) in LDS, a wave owns R = 2 output rows per pass, its 64 lanes stride the
// row in 16-byte chunks (one wave instruction = 1 KiB of q, coalesced, non-temporal) plus the chunk's scale byte (the two lanes of a block read
// the same byte).  The prologues are gemv.hip's, statement for statement, so that h_out is bit-identical to dl_gemv's.
#include <mutex>

#include "act_round.h"
#include "gemv_dot.h"
#include "../../include/dynllava.h"

namespace dl {

constexpr int kMx8Threads = 256;
constexpr int kMx8GridCap = 1024;  // gemv.hip's default: 4 workgroups per CU
constexpr int kMx8MaxB = 8;

typedef float mx_f32x2_t __attribute__((ext_vector_type(2)));

// sum over the 16 weights of one chunk of x * q (q unscaled), fp32.  xs: the 16 x elements (32 bytes for the 16-bit dtypes, 64 for f32) in LDS.
template <typename T>
__device__ __forceinline__ float mx8_dot16(const uint4& w, const typename Elem<T>::storage* xs) {
  const uint32_t wq[4] = {w.x, w.y, w.z, w.w};
  float p = 0.f;
  if constexpr (Elem<T>::kVec == 4) {
    const uint4 x0 = reinterpret_cast<const uint4*>(xs)[0], x1 = reinterpret_cast<const uint4*>(xs)[1];
    const uint4 x2 = reinterpret_cast<const uint4*>(xs)[2], x3 = reinterpret_cast<const uint4*>(xs)[3];
    const uint32_t xw[16] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w, x2.x, x2.y, x2.z, x2.w, x3.x, x3.y, x3.z, x3.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const mx_f32x2_t lo = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(wq[i], 1.0f, false);
      const mx_f32x2_t hi = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(wq[i], 1.0f, true);
      p = fmaf(lo.x, __uint_as_float(xw[4 * i]), p);
      p = fmaf(lo.y, __uint_as_float(xw[4 * i + 1]), p);
      p = fmaf(hi.x, __uint_as_float(xw[4 * i + 2]), p);
      p = fmaf(hi.y, __uint_as_float(xw[4 * i + 3]), p);
    }
  } else {
    const uint4 x0 = reinterpret_cast<const uint4*>(xs)[0], x1 = reinterpret_cast<const uint4*>(xs)[1];
    const uint32_t xw[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (Elem<T>::kBf16) {
        const gv_bf16x2_t lo = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(wq[i], 1.0f, false);
        const gv_bf16x2_t hi = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(wq[i], 1.0f, true);
        p = __builtin_amdgcn_fdot2_f32_bf16(lo, __builtin_bit_cast(gv_bf16x2_t, xw[2 * i]), p, false);
        p = __builtin_amdgcn_fdot2_f32_bf16(hi, __builtin_bit_cast(gv_bf16x2_t, xw[2 * i + 1]), p, false);
      } else {
        const gv_f16x2_t lo = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(wq[i], 1.0f, false);
        const gv_f16x2_t hi = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(wq[i], 1.0f, true);
        p = __builtin_amdgcn_fdot2(lo, __builtin_bit_cast(gv_f16x2_t, xw[2 * i]), p, false);
        p = __builtin_amdgcn_fdot2(hi, __builtin_bit_cast(gv_f16x2_t, xw[2 * i + 1]), p, false);
      }
    }
  }
  return p;
}

// E8M0 code -> 2^(code - 127) as fp32 (codes 1..254; the quantiser writes 3..254)
__device__ __forceinline__ float mx8_scale(uint32_t code) { return __uint_as_float(code << 23); }

// MODE: 0 plain, 1 add + RMSNorm (gemv.hip's prologues).  PAIR: the wave's two rows are (n, n + N/2), epilogue cast(cast(silu(g)) * u).
template <typename T, int B, int MODE, bool PAIR, int R, int U>
__global__ __launch_bounds__(kMx8Threads) void gemv_mx8_kernel(const uint8_t* __restrict__ q, const uint8_t* __restrict__ sc, int N, int K, const void* x_,
                                                               int64_t x_rs, const void* __restrict__ h_, void* __restrict__ h_out_,
                                                               const void* __restrict__ delta_, const void* __restrict__ nw_, float eps,
                                                               void* __restrict__ y_, int64_t y_rs) {
  constexpr int V = Elem<T>::kVec;
  using S = typename Elem<T>::storage;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  S* xs = reinterpret_cast<S*>(smem);  // [B][K] in the model dtype
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int bid = (int)blockIdx.x, nblk = (int)gridDim.x;
  const int nvec = K / V;     // 16-byte chunks of x
  const int nch = K / 16;     // 16-byte chunks of a q row
  const int nsb = K / 32;     // scale bytes of a row

  // ---- start the weight stream before the prologue (as gemv.hip) ----
  const int n_out = PAIR ? N / 2 : N;
  constexpr int RW = PAIR ? 1 : R;
  const int groups = (n_out + 4 * RW - 1) / (4 * RW);
  uint4 pre[R][U];
  uint32_t pre_s[R][U];
  const bool have_pre = bid < groups && lane + 64 * (U - 1) < nch;
  if (have_pre) {
    const int n0 = bid * 4 * RW + wid * RW;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int n = PAIR ? (n0 + r * n_out) : (n0 + r);
      n = n < N ? n : N - 1;
      if (PAIR && n0 >= n_out) n = r * n_out;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int c = lane + 64 * u;
        pre[r][u] = ldg_nt(q + (int64_t)n * K + c * 16);
        pre_s[r][u] = sc[(int64_t)n * nsb + (c >> 1)];
      }
    }
  }

  // ---- prologue: build x in LDS (gemv.hip's gemv_body, unchanged arithmetic) ----
  if constexpr (MODE == 1) {  // ADDNORM
    const S* h = reinterpret_cast<const S*>(h_);
    S* h_out = reinterpret_cast<S*>(h_out_);
    const S* dl_ = reinterpret_cast<const S*>(delta_);
    const S* nw = reinterpret_cast<const S*>(nw_);
    constexpr int MAXC = 4;
    if (nvec <= kMx8Threads * MAXC) {
      uint4 wr[MAXC];
#pragma unroll
      for (int c = 0; c < MAXC; ++c) {
        const int v = tid + c * kMx8Threads;
        if (v < nvec) wr[c] = *reinterpret_cast<const uint4*>(nw + v * V);
      }
#pragma unroll
      for (int b = 0; b < B; ++b) {
        uint4 hr[MAXC], dr[MAXC];
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
          const int v = tid + c * kMx8Threads;
          if (v < nvec) {
            hr[c] = *reinterpret_cast<const uint4*>(h + (int64_t)b * K + v * V);
            if (dl_) dr[c] = *reinterpret_cast<const uint4*>(dl_ + (int64_t)b * K + v * V);
          }
        }
        float a[MAXC][V];
        float ss = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
          const int v = tid + c * kMx8Threads;
          if (v < nvec) {
            unpack16<T>(hr[c], a[c]);
            if (dl_) {
              float d[V];
              unpack16<T>(dr[c], d);
#pragma unroll
              for (int e = 0; e < V; ++e) a[c][e] = Elem<T>::round(a[c][e] + d[e]);
              if (bid == 0) store16<T>(h_out + (int64_t)b * K + v * V, a[c]);
            }
#pragma unroll
            for (int e = 0; e < V; ++e) ss += a[c][e] * a[c][e];
          }
        }
        const float rstd = rsqrtf(block_sum<4>(ss, red) / (float)K + eps);
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
          const int v = tid + c * kMx8Threads;
          if (v < nvec) {
            float w[V];
            unpack16<T>(wr[c], w);
#pragma unroll
            for (int e = 0; e < V; ++e) a[c][e] = w[e] * Elem<T>::round(a[c][e] * rstd);
            store16<T>(xs + b * K + v * V, a[c]);
          }
        }
      }
    } else {
#pragma unroll
      for (int b = 0; b < B; ++b) {
        float ss = 0.f;
        for (int v = tid; v < nvec; v += kMx8Threads) {
          float a[V];
          load16<T>(h + (int64_t)b * K + v * V, a);
          if (dl_) {
            float d[V];
            load16<T>(dl_ + (int64_t)b * K + v * V, d);
#pragma unroll
            for (int e = 0; e < V; ++e) a[e] = Elem<T>::round(a[e] + d[e]);
            if (bid == 0) store16<T>(h_out + (int64_t)b * K + v * V, a);
          }
#pragma unroll
          for (int e = 0; e < V; ++e) ss += a[e] * a[e];
          store16<T>(xs + b * K + v * V, a);
        }
        const float rstd = rsqrtf(block_sum<4>(ss, red) / (float)K + eps);
        for (int v = tid; v < nvec; v += kMx8Threads) {
          float a[V], w[V];
          load16<T>(xs + b * K + v * V, a);
          load16<T>(nw + v * V, w);
#pragma unroll
          for (int e = 0; e < V; ++e) a[e] = w[e] * Elem<T>::round(a[e] * rstd);
          store16<T>(xs + b * K + v * V, a);
        }
      }
    }
  } else {
    const S* x = reinterpret_cast<const S*>(x_);
#pragma unroll
    for (int b = 0; b < B; ++b)
      for (int v = tid; v < nvec; v += kMx8Threads)
        *reinterpret_cast<uint4*>(xs + b * K + v * V) = *reinterpret_cast<const uint4*>(x + (int64_t)b * x_rs + v * V);
  }
  __syncthreads();

  // ---- stream q + scales ----
  bool first = have_pre;
  for (int grp = bid; grp < groups; grp += nblk) {
    const int n0 = grp * 4 * RW + wid * RW;
    float acc[R][B];
    const uint8_t* qp[R];
    const uint8_t* sp[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int b = 0; b < B; ++b) acc[r][b] = 0.f;
      int n = PAIR ? (n0 + r * n_out) : (n0 + r);
      n = n < N ? n : N - 1;
      if (PAIR && n0 >= n_out) n = r * n_out;
      qp[r] = q + (int64_t)n * K;
      sp[r] = sc + (int64_t)n * nsb;
    }
    int c = lane;
    for (; c + 64 * (U - 1) < nch; c += 64 * U) {
      uint4 raw[R][U];
      uint32_t rs[R][U];
      if (first) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int r = 0; r < R; ++r) {
            raw[r][u] = pre[r][u];
            rs[r][u] = pre_s[r][u];
          }
        first = false;
      } else {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int r = 0; r < R; ++r) {
            raw[r][u] = ldg_nt(qp[r] + (c + 64 * u) * 16);
            rs[r][u] = sp[r][(c + 64 * u) >> 1];
          }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int b = 0; b < B; ++b) {
          const S* xc = xs + b * K + (c + 64 * u) * 16;
#pragma unroll
          for (int r = 0; r < R; ++r) acc[r][b] = fmaf(mx8_dot16<T>(raw[r][u], xc), mx8_scale(rs[r][u]), acc[r][b]);
        }
      }
    }
    for (; c < nch; c += 64) {
      uint4 raw[R];
      uint32_t rs[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        raw[r] = ldg_nt(qp[r] + c * 16);
        rs[r] = sp[r][c >> 1];
      }
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const S* xc = xs + b * K + c * 16;
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r][b] = fmaf(mx8_dot16<T>(raw[r], xc), mx8_scale(rs[r]), acc[r][b]);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int b = 0; b < B; ++b) acc[r][b] = wave_sum(acc[r][b]);
    if (lane == 0) {
      if constexpr (PAIR) {
        if (n0 < n_out) {
#pragma unroll
          for (int b = 0; b < B; ++b) {
            const float g = Elem<T>::round(acc[0][b]), u = Elem<T>::round(acc[1][b]);
            // the 16-bit types: act_round.h's guarded fast form (the bits of the exact expression, as dl_silu_mul); fp32: the exact expression
            float sg;
            if constexpr (Elem<T>::kBytes == 2) sg = silu_rounded<T>(g);
            else sg = g / (1.0f + expf(-g));
            store1<T>(y_, (int64_t)b * y_rs + n0, sg * u);
          }
        }
      } else {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int b = 0; b < B; ++b)
            if (n0 + r < N) store1<T>(y_, (int64_t)b * y_rs + n0 + r, acc[r][b]);
      }
    }
  }
}

template <typename T, int B, int MODE, bool PAIR>
static int gemv_mx8_go(const void* q, const void* sc, int N, int K, const void* x, int64_t x_rs, const void* h, void* h_out, const void* delta,
                       const void* nw, float eps, void* y, int64_t y_rs, int grid_cap, hipStream_t st) {
  constexpr int R = 2, U = 4;
  const size_t smem = (size_t)B * K * Elem<T>::kBytes;
  const int n_out = PAIR ? N / 2 : N;
  const int per = 4 * (PAIR ? 1 : R);
  const int groups = (n_out + per - 1) / per;
  const int cap = B == 1 ? grid_cap : (grid_cap / 2 > 0 ? grid_cap / 2 : 1);  // gemv.hip's caps
  const int grid = groups < cap ? groups : cap;
  auto kfn = gemv_mx8_kernel<T, B, MODE, PAIR, R, U>;
  if (smem > 64 * 1024) {
    static std::once_flag once;
    static bool attr_ok = false;
    std::call_once(once, [&] {
      attr_ok = hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024) == hipSuccess;
      if (!attr_ok) (void)hipGetLastError();
    });
    if (!attr_ok) {
      set_error("dl_gemv_mx8: cannot raise the dynamic LDS limit to 152 KiB");
      return DL_ERR_LAUNCH;
    }
  }
  hipLaunchKernelGGL(kfn, dim3((unsigned)grid), dim3(kMx8Threads), smem, st, reinterpret_cast<const uint8_t*>(q), reinterpret_cast<const uint8_t*>(sc), N, K,
                     x, x_rs, h, h_out, delta, nw, eps, y, y_rs);
  return DL_OK;
}

template <typename T, int B>
static int gemv_mx8_launch(int mode, const void* q, const void* sc, int N, int K, const void* x, int64_t x_rs, const void* h, void* h_out,
                           const void* delta, const void* nw, float eps, void* y, int64_t y_rs, int grid_cap, hipStream_t st) {
#define DL_ARGS q, sc, N, K, x, x_rs, h, h_out, delta, nw, eps, y, y_rs, grid_cap, st
  if (mode == (DL_GEMV_ADDNORM | DL_GEMV_OUT_SILU_PAIR)) return gemv_mx8_go<T, B, 1, true>(DL_ARGS);
  if (mode == DL_GEMV_ADDNORM) return gemv_mx8_go<T, B, 1, false>(DL_ARGS);
  return gemv_mx8_go<T, B, 0, false>(DL_ARGS);
#undef DL_ARGS
}

// ---- the quantiser: one thread per 32-element block ----
// exactly mxfp8.py's rule: amax == 0 -> e = 0, q = 0; else e = clamp(floor(log2 amax) - 8, e_min, 127), q = RNE(w / 2^e) to e4m3fn saturated at +-448.
template <typename T>
__global__ __launch_bounds__(256) void quantize_mx8_kernel(const void* __restrict__ w_, int64_t n_blocks, int K, int e_min, uint8_t* __restrict__ q,
                                                           uint8_t* __restrict__ sc, int32_t* __restrict__ err) {
  using S = typename Elem<T>::storage;
  const int64_t blk = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (blk >= n_blocks) return;
  const int nsb = K / 32;
  const int64_t row = blk / nsb, off = row * K + (blk % nsb) * 32;  // element offset of the block
  const S* w = reinterpret_cast<const S*>(w_) + off;
  float v[32];
#pragma unroll
  for (int i = 0; i < 32; i += Elem<T>::kVec) {
    float f[Elem<T>::kVec];
    load16<T>(w + i, f);
#pragma unroll
    for (int j = 0; j < Elem<T>::kVec; ++j) v[i + j] = f[j];
  }
  float amax = 0.f;
  bool bad = false;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    const float a = fabsf(v[i]);
    bad |= !(a <= 3.4028234663852886e38f);  // NaN or Inf
    amax = fmaxf(amax, a);
  }
  if (bad && err) *err = 1;
  int e = 0;
  if (amax > 0.f) {
    const uint32_t ab = __float_as_uint(amax);
    const int ex = (int)(ab >> 23);
    const int fl = ex != 0 ? ex - 127 : (31 - __clz((int)(ab & 0x7fffffu))) - 149;  // floor(log2(amax)), fp32 subnormals included
    e = fl - 8;
    e = e < e_min ? e_min : (e > 127 ? 127 : e);
  }
  // 2^-e as fp32 (e in [-124, 127]): two factors keep both normal (2^-127 is not)
  const float inv_hi = __uint_as_float((uint32_t)(127 - (e >> 1)) << 23), inv_lo = __uint_as_float((uint32_t)(127 - (e - (e >> 1))) << 23);
  uint32_t packed[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) packed[i] = 0u;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    uint32_t code = 0u;
    if (amax > 0.f) {
      const float s = (v[i] * inv_hi) * inv_lo;  // exact unless it underflows fp32 (then it rounds to 0 in e4m3 either way)
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
      code = (sign << 7) | mag;
    }
    packed[i >> 2] |= code << (8 * (i & 3));
  }
  uint4* qo = reinterpret_cast<uint4*>(q + off);
  qo[0] = make_uint4(packed[0], packed[1], packed[2], packed[3]);
  qo[1] = make_uint4(packed[4], packed[5], packed[6], packed[7]);
  sc[blk] = (uint8_t)(e + 127);
}

}  // namespace dl

using namespace dl;

extern "C" int dl_mx8_e_min(int dtype) { return dtype == DL_F16 ? -15 : (dtype == DL_F32 || dtype == DL_BF16) ? -124 : 0; }

extern "C" int dl_quantize_mx8(const void* W, int64_t N, int K, int src_dtype, int model_dtype, void* q, void* scale, int32_t* err_flag, void* stream) {
  DL_REQUIRE(N >= 0 && K > 0 && K % 32 == 0, "dl_quantize_mx8: bad shape N=%lld K=%d (K must be a positive multiple of 32)", (long long)N, K);
  DL_REQUIRE(model_dtype == DL_F32 || model_dtype == DL_F16 || model_dtype == DL_BF16, "dl_quantize_mx8: unsupported model dtype %d", model_dtype);
  if (N == 0) return DL_OK;
  DL_REQUIRE(W && q && scale, "dl_quantize_mx8: NULL pointer");
  const int64_t nb = N * (K / 32);
  const int e_min = dl_mx8_e_min(model_dtype);
  hipStream_t st = as_stream(stream);
  const unsigned grid = (unsigned)((nb + 255) / 256);
  DL_DISPATCH_DTYPE(src_dtype, T, {
    hipLaunchKernelGGL((quantize_mx8_kernel<T>), dim3(grid), dim3(256), 0, st, W, nb, K, e_min, reinterpret_cast<uint8_t*>(q), reinterpret_cast<uint8_t*>(scale), err_flag);
  });
  DL_CHECK_LAUNCH("dl_quantize_mx8");
  return DL_OK;
}

extern "C" int dl_gemv_mx8(int mode, const void* q, const void* scale, int N, int K, const void* x, int64_t x_row_stride, const void* h_in, void* h_out,
                           const void* delta, const void* norm_w, float eps, void* y, int64_t y_row_stride, int B, int dtype, int grid_cap, void* stream) {
  DL_REQUIRE(q && scale && y, "dl_gemv_mx8: NULL pointer");
  DL_REQUIRE(N > 0 && K > 0 && B > 0 && grid_cap >= 0, "dl_gemv_mx8: bad shape");
  DL_REQUIRE(K % 32 == 0, "dl_gemv_mx8: K=%d must be a multiple of 32 (the scale block)", K);
  DL_REQUIRE(dtype == DL_F32 || dtype == DL_F16 || dtype == DL_BF16, "dl_gemv_mx8: unsupported dtype %d", dtype);
  DL_REQUIRE(mode == DL_GEMV_PLAIN || mode == DL_GEMV_ADDNORM || mode == (DL_GEMV_ADDNORM | DL_GEMV_OUT_SILU_PAIR),
             "dl_gemv_mx8: mode %d unsupported (PLAIN, ADDNORM, ADDNORM | OUT_SILU_PAIR)", mode);
  DL_REQUIRE(!(mode & DL_GEMV_OUT_SILU_PAIR) || N % 2 == 0, "dl_gemv_mx8: SILU_PAIR needs an even N");
  const int pro = mode & 3;
  DL_REQUIRE(pro == DL_GEMV_ADDNORM ? (h_in && norm_w) : (x != nullptr), "dl_gemv_mx8: missing operand for mode %d", mode);
  DL_REQUIRE(!(pro == DL_GEMV_ADDNORM && delta) || (h_out && h_out != h_in), "dl_gemv_mx8: h_out must be a distinct buffer when delta is given");
  DL_REQUIRE(B <= kMx8MaxB && B <= dl_gemv_max_batch(K, dtype), "dl_gemv_mx8: B=%d rows of K=%d do not fit in LDS (max %d)", B, K, dl_gemv_max_batch(K, dtype));
  if (grid_cap == 0) grid_cap = kMx8GridCap;
  hipStream_t st = as_stream(stream);
  int rc = DL_OK;
  DL_DISPATCH_DTYPE(dtype, T, {
    DL_REQUIRE(pro == DL_GEMV_ADDNORM || x_row_stride % Elem<T>::kVec == 0, "dl_gemv_mx8: x_row_stride must be a multiple of %d", Elem<T>::kVec);
    switch (B) {
      case 1: rc = gemv_mx8_launch<T, 1>(mode, q, scale, N, K, x, x_row_stride, h_in, h_out, delta, norm_w, eps, y, y_row_stride, grid_cap, st); break;
      case 2: rc = gemv_mx8_launch<T, 2>(mode, q, scale, N, K, x, x_row_stride, h_in, h_out, delta, norm_w, eps, y, y_row_stride, grid_cap, st); break;
      case 3: rc = gemv_mx8_launch<T, 3>(mode, q, scale, N, K, x, x_row_stride, h_in, h_out, delta, norm_w, eps, y, y_row_stride, grid_cap, st); break;
      case 4: rc = gemv_mx8_launch<T, 4>(mode, q, scale, N, K, x, x_row_stride, h_in, h_out, delta, norm_w, eps, y, y_row_stride, grid_cap, st); break;
      case 5: rc = gemv_mx8_launch<T, 5>(mode, q, scale, N, K, x, x_row_stride, h_in, h_out, delta, norm_w, eps, y, y_row_stride, grid_cap, st); break;
      case 6: rc = gemv_mx8_launch<T, 6>(mode, q, scale, N, K, x, x_row_stride, h_in, h_out, delta, norm_w, eps, y, y_row_stride, grid_cap, st); break;
      case 7: rc = gemv_mx8_launch<T, 7>(mode, q, scale, N, K, x, x_row_stride, h_in, h_out, delta, norm_w, eps, y, y_row_stride, grid_cap, st); break;
      default: rc = gemv_mx8_launch<T, 8>(mode, q, scale, N, K, x, x_row_stride, h_in, h_out, delta, norm_w, eps, y, y_row_stride, grid_cap, st); break;
    }
  });
  if (rc != DL_OK) return rc;
  DL_CHECK_LAUNCH("dl_gemv_mx8");
  return DL_OK;
}
