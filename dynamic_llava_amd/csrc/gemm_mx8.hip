// dl_gemm_mx8: Y[M,N] = X[M,K] @ W'[N,K]^T for decode batches 1 <= M <= 32, W' given as MXFP8 (q uint8 [N,K], scale uint8 [N,K/32]) exactly as
// dl_quantize_mx8 writes them -- the decoder's q|k|v, o_proj, gate|up and down_proj when 4..32 rows are decoded together on MXFP8 weights.  These steps are
// weight streaming (M flop per weight byte): 1.03 bytes per weight instead of 2 is the whole point.
//
// Structure: gemm_smallm.hip's LDS-staged kernel on one byte per weight.
//  * X (one K slice, model dtype) is RESIDENT in LDS ([16*NB rows][Ks + 8]); K is split over gridDim.y slices, fp32 partial sums go to the workspace and are
//    added in slice order (splitk_reduce.h) or left there for dl_add_rmsnorm_parts / dl_silu_mul_parts (DL_MX8_PARTS).
//  * a WAVE owns 16 neurons at a time and streams their codes in chunks of [16 neurons x 256 k] = 4 KiB: four coalesced non-temporal 16-byte loads per lane
//    (one instruction = 4 rows x 256 contiguous bytes) plus the chunk's 8 scale bytes of neuron (lane & 15); FOUR chunks (16 KiB) are in flight per wave.
//    A chunk is parked in wave-private LDS (rows of 256 + 16 bytes: the 8-byte fragment reads below are conflict-free; no barrier, only the wave reads it
//    back) and read back as MFMA A-fragments: lane (r = lane & 15, g = lane >> 4) takes the 8 codes of neuron r at k = 32 b + 8 g, so every K = 32 MFMA covers
//    exactly ONE scale block b for all four lane groups.
//  * numerics: the codes are converted AT UNIT SCALE with v_cvt_scalef32_pk_{bf16,f16}_fp8 (every e4m3 value is a normal bf16 / fp16 number), each
//    v_mfma_f32_16x16x32 runs into a ZERO accumulator (p = the fp32 sum of the exact products x * q over one block) and the block exponent is applied with one
//    fp32 FMA per accumulator register: acc = fma(p, 2^e, acc).  A power of two commutes with fp32 rounding, so this is the fp32 sum of exact products with
//    W', rounded once to the output dtype -- dl_gemv_mx8's contract.  2^e never enters the conversion or the MFMA inputs, so the dtype's subnormals that W'
//    contains (fp16 blocks at e = -15 hold many) never meet an instruction whose subnormal handling is undocumented; tests/test_mxfp8_batched_gpu.py checks
//    all 256 codes x every exponent bit for bit.  D[neuron = 4 g + i][batch row = r]: a lane needs the scales of its 4 D neurons, 8 bytes each per chunk =
//    32 contiguous bytes of the wave's staged [16 neurons][8] scale bytes.
#include "dl_common.h"
#include "splitk_reduce.h"
#include "../../include/dynllava.h"

namespace dl {

typedef __bf16 mg_bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 mg_bf16x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 mg_f16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 mg_f16x2_t __attribute__((ext_vector_type(2)));
typedef float mg_f32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t mg_u32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t mg_u32x2_t __attribute__((ext_vector_type(2)));

constexpr int kMgKUnit = 256;                        // K slices are multiples of the chunk length
constexpr int kMgKC = 256;                           // k per chunk
constexpr int kMgMaxM = 32;
constexpr int kMgWaves = 8;                          // waves per workgroup
constexpr int kMgRowBytes = kMgKC + 16;              // staged code row: +16 bytes -> rows shift by 4 banks
constexpr int kMgStageBytes = 16 * kMgRowBytes + 16 * 8;  // per wave: codes [16][272] + scales [16][8]
constexpr int kMgLdsBytes = 150 * 1024;

// 8 e4m3 codes (two dwords) -> 8 values of T at unit scale, in k order, as an MFMA operand
template <typename T>
__device__ __forceinline__ mg_u32x4_t mg_cvt8(mg_u32x2_t c) {
  if constexpr (Elem<T>::kBf16) {
    return mg_u32x4_t{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c.x, 1.0f, false)),
                      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c.x, 1.0f, true)),
                      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c.y, 1.0f, false)),
                      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c.y, 1.0f, true))};
  } else {
    return mg_u32x4_t{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c.x, 1.0f, false)),
                      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c.x, 1.0f, true)),
                      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c.y, 1.0f, false)),
                      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c.y, 1.0f, true))};
  }
}

template <typename T>
__device__ __forceinline__ mg_f32x4_t mg_mfma(mg_u32x4_t a, mg_u32x4_t b) {  // one scale block: into a zero accumulator
  const mg_f32x4_t z{0.f, 0.f, 0.f, 0.f};
  if constexpr (Elem<T>::kBf16)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(mg_bf16x8_t, a), __builtin_bit_cast(mg_bf16x8_t, b), z, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(mg_f16x8_t, a), __builtin_bit_cast(mg_f16x8_t, b), z, 0, 0, 0);
}

struct MgChunk {      // one chunk in flight: this lane's share of [16 neurons x 256 codes] and of its scales
  mg_u32x4_t w[4];    // rows 4 j + (lane >> 4), 16 codes at (lane & 15) * 16
  mg_u32x2_t s;       // the chunk's 8 scale bytes of neuron (lane & 15)
};

// NB: batch tiles of 16 rows (M <= 16 * NB)
template <typename T, int NB>
__global__ __launch_bounds__(kMgWaves * 64) void gemm_mx8_kernel(const void* __restrict__ X_, int64_t ldx, const uint8_t* __restrict__ q,
                                                                  const uint8_t* __restrict__ sc, void* __restrict__ Y_, int64_t ldy,
                                                                  float* __restrict__ part, int M, int N, int K, int n_slices, int direct) {
  using S = uint16_t;
  extern __shared__ __attribute__((aligned(16))) unsigned char mg_smem[];
  const S* X = reinterpret_cast<const S*>(X_);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int units = K / kMgKUnit, nsb = K / 32;
  const int slice = blockIdx.y;
  const int u0 = (int)((int64_t)units * slice / n_slices), u1 = (int)((int64_t)units * (slice + 1) / n_slices);
  const int k0 = u0 * kMgKUnit, Ks = (u1 - u0) * kMgKUnit;
  const int ld = Ks + 8;       // X row stride in LDS (elements): +16 bytes -> rows shift by 4 banks
  const int cpt = Ks / kMgKC;  // chunks per tile
  unsigned char* stg = mg_smem + wid * kMgStageBytes;  // wave-private: codes [16][kMgRowBytes], then scales [16][8]
  unsigned char* stg_s = stg + 16 * kMgRowBytes;
  S* xs = reinterpret_cast<S*>(mg_smem + kMgWaves * kMgStageBytes);  // X slice [NB*16][ld]

  const int n_tiles = (N + 15) / 16;
  const int first = blockIdx.x * kMgWaves + wid, stride = gridDim.x * kMgWaves;
  const int my_tiles = first < n_tiles ? (n_tiles - first + stride - 1) / stride : 0;
  const int total = my_tiles * cpt;  // linear (tile, chunk) stream of this wave

  const int scol = lr * 16;  // staging-load role of this lane: rows 4 j + lg, 16 bytes at scol
  auto issue = [&](int t, MgChunk& r) {
    const int tile_i = t / cpt, c = t - tile_i * cpt;
    const int n0 = (first + tile_i * stride) * 16;
    const int kc = k0 + c * kMgKC;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int n = n0 + 4 * j + lg;
      n = n < N ? n : N - 1;  // (rows past N are loaded from the last row and never stored)
      r.w[j] = __builtin_nontemporal_load(reinterpret_cast<const mg_u32x4_t*>(q + (int64_t)n * K + kc + scol));
    }
    int n = n0 + lr;
    n = n < N ? n : N - 1;
    r.s = *reinterpret_cast<const mg_u32x2_t*>(sc + (int64_t)n * nsb + (kc >> 5));
  };

  // ---- start the weight stream before X is staged ----
  MgChunk r0, r1, r2, r3;
  if (total > 0) issue(0, r0);
  if (total > 1) issue(1, r1);
  if (total > 2) issue(2, r2);
  if (total > 3) issue(3, r3);

  {  // X slice -> LDS (rows >= M are zero)
    const int chunks_per_row = Ks / 8;
    const int n_chunks = NB * 16 * chunks_per_row;
    for (int c = tid; c < n_chunks; c += kMgWaves * 64) {
      const int row = c / chunks_per_row, col = (c - row * chunks_per_row) * 8;
      mg_u32x4_t v{0u, 0u, 0u, 0u};
      if (row < M) v = *reinterpret_cast<const mg_u32x4_t*>(X + (int64_t)row * ldx + k0 + col);
      *reinterpret_cast<mg_u32x4_t*>(xs + row * ld + col) = v;
    }
  }
  __syncthreads();

  float acc[NB][4];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[nb][i] = 0.f;
  const S* xb = xs + lr * ld + lg * 8;
  const unsigned char* ab = stg + lr * kMgRowBytes + lg * 8;
  int ci = 0, ti = 0;  // chunk within the tile, tile index

  auto consume = [&](MgChunk& r, int t_next) {
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<mg_u32x4_t*>(stg + (4 * j + lg) * kMgRowBytes + scol) = r.w[j];
    if (lane < 16) *reinterpret_cast<mg_u32x2_t*>(stg_s + lr * 8) = r.s;
    if (t_next < total) issue(t_next, r);
    // the scale bytes of this lane's D neurons 4 lg + i: sw[2 i] holds blocks 0..3, sw[2 i + 1] blocks 4..7
    const mg_u32x4_t s01 = *reinterpret_cast<const mg_u32x4_t*>(stg_s + lg * 32), s23 = *reinterpret_cast<const mg_u32x4_t*>(stg_s + lg * 32 + 16);
    const uint32_t sw[8] = {s01.x, s01.y, s01.z, s01.w, s23.x, s23.y, s23.z, s23.w};
#pragma unroll
    for (int b = 0; b < kMgKC / 32; ++b) {
      const mg_u32x4_t a = mg_cvt8<T>(*reinterpret_cast<const mg_u32x2_t*>(ab + b * 32));
      float e2[4];  // 2^e of the 4 neurons (E8M0 code << 23; the quantiser writes codes 3..254)
#pragma unroll
      for (int i = 0; i < 4; ++i) e2[i] = __uint_as_float(((sw[2 * i + (b >> 2)] >> (8 * (b & 3))) & 0xffu) << 23);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const mg_u32x4_t x = *reinterpret_cast<const mg_u32x4_t*>(xb + nb * 16 * ld + ci * kMgKC + b * 32);
        const mg_f32x4_t p = mg_mfma<T>(a, x);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[nb][i] = fmaf(p[i], e2[i], acc[nb][i]);
      }
    }
    if (++ci == cpt) {  // tile finished: D[neuron = lg*4 + i][batch = lr]
      const int n = (first + ti * stride) * 16 + lg * 4;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const int m = nb * 16 + lr;
        if (m < M && n < N) {  // N % 4 == 0: a lane's 4 neurons are all inside or all outside
          if (direct) {
#pragma unroll
            for (int i = 0; i < 4; ++i) store1<T>(Y_, (int64_t)m * ldy + n + i, acc[nb][i]);
          } else {
            *reinterpret_cast<float4*>(part + ((int64_t)slice * M + m) * N + n) = make_float4(acc[nb][0], acc[nb][1], acc[nb][2], acc[nb][3]);
          }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[nb][i] = 0.f;
      }
      ci = 0;
      ++ti;
    }
  };

  for (int t = 0; t < total; t += 4) {
    consume(r0, t + 4);
    if (t + 1 < total) consume(r1, t + 5);
    if (t + 2 < total) consume(r2, t + 6);
    if (t + 3 < total) consume(r3, t + 7);
  }
}

// slices: enough to (a) fit the X slice in LDS beside the staging and (b) give every CU's eight waves a short stream each (dl_gemm_smallm's staged rule)
static int mg_slices(int M, int N, int K, int want) {
  const int units = K / kMgKUnit;
  const int rows = M <= 16 ? 16 : 32;
  const int budget = kMgLdsBytes - kMgWaves * kMgStageBytes;
  const int max_ks = (budget / (rows * 2) - 8) / kMgKUnit * kMgKUnit;
  int s_lds = 1;
  while ((units + s_lds - 1) / s_lds * kMgKUnit > max_ks) ++s_lds;
  int s = want;
  if (s <= 0) s = (N + 15) / 16 >= 1024 ? 4 : 8;
  if (s < s_lds) s = s_lds;
  if (s > units) s = units;
  return s;
}

template <typename T, int NB>
static int mg_go(const void* X, int64_t ldx, const void* q, const void* sc, void* Y, int64_t ldy, float* part, int M, int N, int K, int n_slices,
                 int direct, hipStream_t st) {
  const int units = K / kMgKUnit;
  const int max_ks = (units + n_slices - 1) / n_slices * kMgKUnit;
  const size_t smem = (size_t)kMgWaves * kMgStageBytes + (size_t)NB * 16 * (max_ks + 8) * 2;
  auto kfn = gemm_mx8_kernel<T, NB>;
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024) != hipSuccess) {
      (void)hipGetLastError();
      set_error("dl_gemm_mx8: cannot raise the dynamic LDS limit to 152 KiB");
      return DL_ERR_LAUNCH;
    }
    attr_set = true;
  }
  const int n_tiles = (N + 15) / 16;
  int gx = (n_tiles + kMgWaves - 1) / kMgWaves;
  const int cap = 256 / n_slices > 0 ? 256 / n_slices : 1;  // one workgroup per CU in a single round; tiles beyond that are looped over
  if (gx > cap) gx = cap;
  hipLaunchKernelGGL(kfn, dim3((unsigned)gx, (unsigned)n_slices), dim3(kMgWaves * 64), smem, st, X, ldx, reinterpret_cast<const uint8_t*>(q),
                     reinterpret_cast<const uint8_t*>(sc), Y, ldy, part, M, N, K, n_slices, direct);
  return DL_OK;
}

static bool mg_shape_ok(int M, int N, int K) { return M > 0 && M <= kMgMaxM && N > 0 && K > 0 && K % kMgKUnit == 0 && N % 4 == 0; }

}  // namespace dl

using namespace dl;

extern "C" int dl_gemm_mx8_slices(int M, int N, int K, int n_slices) {
  if (!mg_shape_ok(M, N, K) || n_slices < 0 || n_slices > 64) return 0;
  return mg_slices(M, N, K, n_slices);
}

extern "C" int64_t dl_gemm_mx8_workspace_bytes(int M, int N, int K, int n_slices) {
  const int s = dl_gemm_mx8_slices(M, N, K, n_slices);
  return (int64_t)s * M * N * (int64_t)sizeof(float);  // also covers DL_MX8_PARTS with a single slice
}

extern "C" int dl_gemm_mx8(const void* X, int64_t ldx, const void* q, const void* scale, void* Y, int64_t ldy, void* workspace, int64_t workspace_bytes,
                           int M, int N, int K, int n_slices, int epilogue, int dtype, void* stream) {
  DL_REQUIRE(epilogue == DL_MX8_PLAIN || epilogue == DL_MX8_PARTS, "dl_gemm_mx8: epilogue %d unsupported (DL_MX8_PLAIN, DL_MX8_PARTS)", epilogue);
  const bool parts = epilogue == DL_MX8_PARTS;
  DL_REQUIRE(X && q && scale && (Y || parts), "dl_gemm_mx8: NULL pointer");
  DL_REQUIRE(M > 0 && M <= kMgMaxM && N > 0 && K > 0, "dl_gemm_mx8: bad shape M=%d (max %d) N=%d K=%d", M, kMgMaxM, N, K);
  DL_REQUIRE(dtype == DL_BF16 || dtype == DL_F16, "dl_gemm_mx8: bf16 / f16 only (MFMA path)");
  DL_REQUIRE(K % kMgKUnit == 0 && N % 4 == 0 && ldx % 8 == 0, "dl_gemm_mx8: K %% 256, N %% 4 and ldx %% 8 must be 0");
  DL_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)q & 15) == 0 && ((uintptr_t)scale & 7) == 0, "dl_gemm_mx8: X and q must be 16-byte aligned, scale 8-byte aligned");
  DL_REQUIRE(n_slices >= 0 && n_slices <= 64, "dl_gemm_mx8: n_slices must be in [0, 64]");
  const int s = mg_slices(M, N, K, n_slices);
  const int direct = (s == 1 && !parts) ? 1 : 0;
  DL_REQUIRE(direct || (workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= (int64_t)s * M * N * (int64_t)sizeof(float)),
             "dl_gemm_mx8: a 16-byte aligned workspace of dl_gemm_mx8_workspace_bytes() = %lld bytes is required (got %lld)",
             (long long)((int64_t)s * M * N * (int64_t)sizeof(float)), (long long)workspace_bytes);
  hipStream_t st = as_stream(stream);
  float* part = reinterpret_cast<float*>(workspace);
  int rc;
#define DL_MG_ARGS X, ldx, q, scale, Y, ldy, part, M, N, K, s, direct, st
  if (dtype == DL_BF16) rc = M <= 16 ? mg_go<bf16_t, 1>(DL_MG_ARGS) : mg_go<bf16_t, 2>(DL_MG_ARGS);
  else rc = M <= 16 ? mg_go<f16_t, 1>(DL_MG_ARGS) : mg_go<f16_t, 2>(DL_MG_ARGS);
#undef DL_MG_ARGS
  if (rc != DL_OK) return rc;
  if (!parts) {
    if (dtype == DL_BF16) sm_reduce<bf16_t>(part, Y, ldy, M, N, s, st); else sm_reduce<f16_t>(part, Y, ldy, M, N, s, st);
  }
  DL_CHECK_LAUNCH("dl_gemm_mx8");
  return DL_OK;
}
