// The MXFP8 KV cache (opt-in, cache.py KVSlabCacheMX8): keys (after RoPE) and values stored as e4m3fn codes with one E8M0 scale byte per
// 32 consecutive elements of a row -- the format of mxfp8.py applied along head_dim, in separate planes:
//   codes  uint8 [B, nKV, T_cap, d]      scales uint8 [B, nKV, T_cap, d/32]      (for K and for V; d + d/32 bytes per row instead of 2 d)
//
//   dl_kv_quantize_mx8      -- row ranges of a model-dtype slab -> the planes, bit-exact to mxfp8.quantize_mx8 (the prefill's append)
//   dl_attn_decode_rope_kv8 -- dl_attn_decode_rope's job on the planes: RoPE of q / the new key (DML:260-285), quantised append at slot
//                              kv_len[b] (CU:109-268), ragged split-KV attention over keys [0, kv_len[b]] (DML:1061-1122)
//
// Numerics.  A slab row is read as K' = q * 2^e (V' likewise), exactly: the 16 codes a lane holds (half a scale block) are converted at unit
// scale with v_cvt_scalef32_pk_f32_fp8 (exact), their dot product with the rotated query is accumulated in fp32, and the block's 2^e is applied
// to that fp32 partial (a power of two commutes with the rounding); for V it is applied to the softmax weight, p * 2^e, before the fp32 FMA
// with the unit-scale codes.  No 16-bit subnormal is ever formed.  The NEW token is attended at model-dtype precision -- its rotated key and
// its value are in registers -- and stored quantised, so the launch computes attention over [dequantised old rows | exact new row].
// Everything else is attn_decode_body.h's: fp32 online softmax per lane group, LDS merge of the lane groups, split partials in the workspace
// layout of dl_attn_decode_workspace_bytes merged by attn_decode_combine_kernel, one rounding of the output.
//
// Mapping.  A lane holds 16 bytes = 16 elements of a row, so D/16 lanes (8 at head_dim 128) share a key, a wave-wide load is 64 / (D/16) full rows
// and two neighbouring lanes share one scale byte.  With the bf16 kernel's (NW, U) a trip therefore requests twice the keys and the same bytes
// (half the bytes in flight do not cover the HBM latency).  The scale bytes are requested with the codes, never after them.
// A masked or speculatively read slot may hold any bytes (code 0x7f and scale 0xff are NaN / Inf): its score and its P.V term are SELECTED away,
// never multiplied by zero.
#include "attn_decode_body.h"
#include "mx8_quant.h"

namespace dl {

constexpr int kKv8E = 16;  // elements (code bytes) per lane

typedef float kv8_f32x2_t __attribute__((ext_vector_type(2)));

// 16 e4m3fn codes -> fp32 at unit scale
__device__ __forceinline__ void kv8_unpack(const uint4& r, float (&f)[kKv8E]) {
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const kv8_f32x2_t lo = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[i], 1.0f, false);
    const kv8_f32x2_t hi = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[i], 1.0f, true);
    f[4 * i] = lo.x;
    f[4 * i + 1] = lo.y;
    f[4 * i + 2] = hi.x;
    f[4 * i + 3] = hi.y;
  }
}

// 16 consecutive model-dtype elements: the q / k / v / RoPE-table slice of a lane that holds 16 codes (load16 reads one 16-byte vector, 8 or 4 elements: the
// model-dtype kernels' lane width, so attn_decode_body.h has no wider load to share)
template <typename T>
__device__ __forceinline__ void kv8_load_row(const typename Elem<T>::storage* p, float (&f)[kKv8E]) {
  constexpr int V = Elem<T>::kVec;
#pragma unroll
  for (int j = 0; j < kKv8E / V; ++j) {
    float t[V];
    load16<T>(p + j * V, t);
#pragma unroll
    for (int i = 0; i < V; ++i) f[j * V + i] = t[i];
  }
}

// The row format of the planes, for the stages of attn_decode_body.h (the policy described there).  stride_b / stride_h are the code planes' (bytes =
// elements); the scale planes' are 1/32 of them.  The scale byte of the lane's block is requested with the codes, never after them.
struct KvMx8Rows {
  static constexpr int E = kKv8E;
  static constexpr int kMergeRegsNG = 32;  // 64 lane groups' partials in registers take the kernel from 150 to 166 VGPRs, of the 168 that keep 3 waves per SIMD
  struct Slab {
    uint8_t* codes;  // writable: the kernel appends the new token's row through the same lane pointers
    uint8_t* scales;
  };
  using Ptr = Slab;
  struct Raw {
    uint4 q;     // 16 codes
    uint32_t e;  // the scale byte of their block
  };
  static __device__ __forceinline__ Ptr at(const Slab& s, int64_t stride_b, int64_t stride_h, int b, int kvh, int c) {
    return Ptr{s.codes + (int64_t)b * stride_b + (int64_t)kvh * stride_h + c, s.scales + (int64_t)b * (stride_b >> 5) + (int64_t)kvh * (stride_h >> 5) + (c >> 5)};
  }
  static __device__ __forceinline__ void request(const Ptr& kb, const Ptr& vb, int64_t key, int D, Raw& k, Raw& v) {
    k.q = kv_ld16(kb.codes + key * D);
    v.q = kv_ld16(vb.codes + key * D);
    k.e = kb.scales[key * (D / 32)];
    v.e = vb.scales[key * (D / 32)];
  }
  static __device__ __forceinline__ void unpack(const Raw& r, float (&f)[E]) { kv8_unpack(r.q, f); }
  static __device__ __forceinline__ float dot(const float (&q)[E], const float (&kx)[E], const Raw& r) {
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < E; ++i) a = fmaf(q[i], kx[i], a);
    return a * mx8_pow2(r.e);  // the block's 2^e on the fp32 partial
  }
  static __device__ __forceinline__ void axpy(bool ok, float p, const float (&vx)[E], const Raw& r, float (&o)[E]) {
    const float ps = p * mx8_pow2(r.e);  // p * 2^e: exact
#pragma unroll
    for (int i = 0; i < E; ++i) o[i] = ok ? fmaf(ps, vx[i], o[i]) : o[i];
  }
};

// quantise the 16 elements this lane holds of a row (its neighbour, lane ^ 1, holds the other half of the scale block) and store codes + scale byte
template <int D>
__device__ __forceinline__ void kv8_store_row(const float (&x)[kKv8E], int e_min, uint8_t* codes, uint8_t* scale_byte, bool writes_scale) {
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < kKv8E; ++i) amax = fmaxf(amax, fabsf(x[i]));
  amax = fmaxf(amax, dpp_f32<kDppXor1>(amax));
  const int e = mx8_block_exp(amax, e_min);
  float inv_hi, inv_lo;
  mx8_inv_scale(e, inv_hi, inv_lo);
  uint32_t packed[4] = {0u, 0u, 0u, 0u};
  if (amax > 0.f) {
#pragma unroll
    for (int i = 0; i < kKv8E; ++i) packed[i >> 2] |= mx8_code(x[i], inv_hi, inv_lo) << (8 * (i & 3));
  }
  *reinterpret_cast<uint4*>(codes) = make_uint4(packed[0], packed[1], packed[2], packed[3]);
  if (writes_scale) *scale_byte = (uint8_t)(e + 127);
}

// grid (n_splits, n_heads, B), NW waves.  attn_decode_split_kernel's sequence with its own finish: the new token opens its lane group's softmax.
template <typename T, int D, int NW, int U>
__global__ __launch_bounds__(NW * 64) void attn_decode_kv8_kernel(
    const void* __restrict__ qkv_, int64_t q_row_stride, uint8_t* kq_, uint8_t* ksc_, uint8_t* vq_, uint8_t* vsc_, int64_t stride_b, int64_t stride_h,
    const int32_t* __restrict__ kv_len, float* __restrict__ ws, void* __restrict__ out_, int64_t out_row_stride, int n_rep, float scale,
    const void* __restrict__ cos_, const void* __restrict__ sin_, int n_pos, const int32_t* __restrict__ pos_base, int T_cap, int n_kv_heads, int chunk_keys,
    int e_min) {
  using St = AttnSplitState<T, D, NW, U, KvMx8Rows>;
  using S = typename Elem<T>::storage;
  constexpr int E = St::E, LPK = St::LPK, NG = St::NG, HALF = D / 2, NSB = D / 32;
  static_assert(NW * 64 >= D, "the D finishing threads");
  __shared__ float sm_m[NG], sm_l[NG];
  __shared__ __attribute__((aligned(16))) float sm_o[NG * D];

  const int split = blockIdx.x, n_splits = gridDim.x, h = blockIdx.y;
  const int n_heads = gridDim.y;
  const int tid = threadIdx.x;
  int b, T_ranked;  // ragged batches, longest row first
  attn_rank_row(kv_len, b, T_ranked);
  const int kvh = h / n_rep;
  const int T_old = T_ranked >= 0 ? T_ranked : kv_len[b];
  St st;
  attn_split_issue<T, D, NW, true, U>(st, tid, KvMx8Rows::Slab{kq_, ksc_}, KvMx8Rows::Slab{vq_, vsc_}, stride_b, stride_h, T_old, 1, b, kvh, split, n_splits, T_cap,
                                      chunk_keys);

  // ---- RoPE of q; the new token's key / value for the lane group that owns key index T_old ----
  const char* row = reinterpret_cast<const char*>(qkv_) + (int64_t)b * q_row_stride * (int64_t)sizeof(S);
  const S* qrow = reinterpret_cast<const S*>(row) + (int64_t)h * D;
  const S* krow = reinterpret_cast<const S*>(row) + (int64_t)(n_heads + kvh) * D;
  const S* vrow = reinterpret_cast<const S*>(row) + (int64_t)(n_heads + n_kv_heads + kvh) * D;
  const int c = st.c;
  const bool upper = c >= HALF;
  const int cpar = upper ? c - HALF : c + HALF;
  const bool owns_new = T_old >= st.k0 && T_old < st.k1s && st.wid == 0 && st.g == 0;
  float qv[E], cs[E], sn[E], kn[E], vn[E];
  {
    int p = pos_base[b];
    p = p < 0 ? 0 : (p >= n_pos ? n_pos - 1 : p);
    float own[E], par[E];
    kv8_load_row<T>(reinterpret_cast<const S*>(cos_) + (int64_t)p * D + (c % HALF), cs);  // table = cat(freqs, freqs)
    kv8_load_row<T>(reinterpret_cast<const S*>(sin_) + (int64_t)p * D + (c % HALF), sn);
    kv8_load_row<T>(qrow + c, own);
    if (owns_new) {
      float kown[E], kpar[E];
      kv8_load_row<T>(krow + c, kown);
      kv8_load_row<T>(krow + cpar, kpar);
      kv8_load_row<T>(vrow + c, vn);
      rope16<T>(upper, kown, kpar, cs, sn, kn);
    }
    // q's partner half (column c +- D/2) is what the lane LPK / 2 lanes away in this lane group has just loaded
#pragma unroll
    for (int i = 0; i < E; ++i) par[i] = __shfl_xor(own[i], LPK / 2);
    rope16<T>(upper, own, par, cs, sn, qv);
  }

  // ---- online softmax per lane group (m, l, o[16]) ----
  float m, l, o[E];
  attn_softmax_open(m, l, o);
  // the new token (key index T_old) opens its lane group's softmax: exact in the model dtype for this step, stored quantised for the later ones.  (Folding it
  // in before the slab keys instead of after them -- attn_split_finish's order -- frees its 32 registers for the loop and puts the quantiser under the first
  // trip's memory latency; the online softmax gives the same value up to fp32 rounding.)
  if (owns_new) {
    if (h % n_rep == 0 && T_old < T_cap) {  // one writer per kv head; eviction = the length is simply not advanced later
      const bool writes_scale = (st.lane & 1) == 0;
      kv8_store_row<D>(kn, e_min, st.kb.codes + (int64_t)T_old * D, st.kb.scales + (int64_t)T_old * NSB, writes_scale);
      kv8_store_row<D>(vn, e_min, st.vb.codes + (int64_t)T_old * D, st.vb.scales + (int64_t)T_old * NSB, writes_scale);
    }
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < E; ++i) a = fmaf(qv[i], kn[i], a);
    a = lpk_sum<LPK>(a);
    m = a * scale;
    l = 1.f;
#pragma unroll
    for (int i = 0; i < E; ++i) o[i] = vn[i];
  }
  attn_split_keys(st, qv, scale, m, l, o);  // the slab keys [k0, k1)

  float M, L, O;
  attn_split_lds_merge(st, tid, m, l, o, sm_m, sm_l, sm_o, M, L, O);
  if (tid < D) attn_store_partial<T, D>(tid, b, h, n_heads, split, n_splits, M, L, O, ws, out_, out_row_stride);
}

template <typename T, int D, int NW, int U>
static void launch_kv8(const void* qkv, int64_t q_row_stride, void* kq, void* ksc, void* vq, void* vsc, int64_t stride_b, int64_t stride_h, const int32_t* kv_len,
                       void* out, int64_t out_row_stride, void* workspace, int n_splits, int B, int n_heads, int n_kv_heads, const void* cos_tab, const void* sin_tab,
                       int n_pos, const int32_t* pos_base, int T_cap, int chunk_keys, int e_min, hipStream_t st) {
  const float scale = 1.0f / sqrtf((float)D);
  hipLaunchKernelGGL((attn_decode_kv8_kernel<T, D, NW, U>), dim3((unsigned)n_splits, (unsigned)n_heads, (unsigned)B), dim3(NW * 64), 0, st, qkv, q_row_stride,
                     reinterpret_cast<uint8_t*>(kq), reinterpret_cast<uint8_t*>(ksc), reinterpret_cast<uint8_t*>(vq), reinterpret_cast<uint8_t*>(vsc), stride_b, stride_h,
                     kv_len, reinterpret_cast<float*>(workspace), out, out_row_stride, n_heads / n_kv_heads, scale, cos_tab, sin_tab, n_pos, pos_base, T_cap, n_kv_heads,
                     chunk_keys, e_min);
  if (n_splits > 1)
    hipLaunchKernelGGL((attn_decode_combine_kernel<T, D>), dim3((unsigned)n_heads, (unsigned)B), dim3(D), 0, st, reinterpret_cast<const float*>(workspace), out,
                       out_row_stride, n_splits);
}

// ---- the quantiser of slab rows: one thread per 32-element block of a K or V row ----
// grid (ceil(max_tokens * 2 * d/32 / 256), nKV, B).  Row b: tokens j in [0, cu[b+1] - cu[b]) at slot kv_base[b] + j of BOTH slabs.
template <typename T>
__global__ __launch_bounds__(256) void kv_quantize_mx8_kernel(const void* __restrict__ k_src, const void* __restrict__ v_src, int64_t src_stride_b, int64_t src_stride_h,
                                                              int src_T_cap, uint8_t* __restrict__ kq, uint8_t* __restrict__ ksc, uint8_t* __restrict__ vq,
                                                              uint8_t* __restrict__ vsc, int64_t dst_stride_b, int64_t dst_stride_h, int dst_T_cap,
                                                              const int32_t* __restrict__ cu, const int32_t* __restrict__ kv_base, int d, int e_min,
                                                              int32_t* __restrict__ err) {
  using S = typename Elem<T>::storage;
  constexpr int V = Elem<T>::kVec;
  const int b = blockIdx.z, h = blockIdx.y;
  const int n_tok = cu[b + 1] - cu[b];
  const int nsb = d / 32;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)n_tok * 2 * nsb) return;
  const int blk = (int)(idx % nsb), which = (int)((idx / nsb) & 1);
  const int64_t slot = (int64_t)kv_base[b] + idx / (2 * nsb);
  if (slot < 0 || slot >= src_T_cap || slot >= dst_T_cap) return;  // a write at or past the capacity is dropped
  const S* src = reinterpret_cast<const S*>(which ? v_src : k_src) + (int64_t)b * src_stride_b + (int64_t)h * src_stride_h + slot * d + blk * 32;
  float v[32];
#pragma unroll
  for (int i = 0; i < 32; i += V) {
    float f[V];
    load16<T>(src + i, f);
#pragma unroll
    for (int j = 0; j < V; ++j) v[i + j] = f[j];
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
  const int e = mx8_block_exp(amax, e_min);
  float inv_hi, inv_lo;
  mx8_inv_scale(e, inv_hi, inv_lo);
  uint32_t packed[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  if (amax > 0.f) {
#pragma unroll
    for (int i = 0; i < 32; ++i) packed[i >> 2] |= mx8_code(v[i], inv_hi, inv_lo) << (8 * (i & 3));
  }
  const int64_t row = (int64_t)b * dst_stride_b + (int64_t)h * dst_stride_h + slot * d;
  uint4* qo = reinterpret_cast<uint4*>((which ? vq : kq) + row + blk * 32);
  qo[0] = make_uint4(packed[0], packed[1], packed[2], packed[3]);
  qo[1] = make_uint4(packed[4], packed[5], packed[6], packed[7]);
  (which ? vsc : ksc)[(int64_t)b * (dst_stride_b >> 5) + (int64_t)h * (dst_stride_h >> 5) + slot * nsb + blk] = (uint8_t)(e + 127);
}

}  // namespace dl

using namespace dl;

extern "C" int dl_kv_quantize_mx8(const void* k_src, const void* v_src, int64_t src_stride_b, int64_t src_stride_h, int src_T_cap, void* k_codes, void* k_scales,
                                  void* v_codes, void* v_scales, int64_t dst_stride_b, int64_t dst_stride_h, int dst_T_cap, const int32_t* cu_seqlens,
                                  const int32_t* kv_base, int max_tokens, int B, int n_kv_heads, int head_dim, int src_dtype, int model_dtype, int32_t* err_flag,
                                  void* stream) {
  DL_REQUIRE(B > 0 && n_kv_heads > 0 && max_tokens >= 0 && src_T_cap > 0 && dst_T_cap > 0, "dl_kv_quantize_mx8: bad shape");
  DL_REQUIRE(head_dim > 0 && head_dim % 32 == 0, "dl_kv_quantize_mx8: head_dim=%d must be a positive multiple of 32 (the scale block)", head_dim);
  DL_REQUIRE(model_dtype == DL_F32 || model_dtype == DL_F16 || model_dtype == DL_BF16, "dl_kv_quantize_mx8: unsupported model dtype %d", model_dtype);
  DL_REQUIRE(src_dtype == DL_F32 || src_dtype == DL_F16 || src_dtype == DL_BF16, "dl_kv_quantize_mx8: unsupported source dtype %d", src_dtype);
  if (max_tokens == 0) return DL_OK;
  DL_REQUIRE(k_src && v_src && k_codes && k_scales && v_codes && v_scales && cu_seqlens && kv_base, "dl_kv_quantize_mx8: NULL pointer");
  DL_REQUIRE(dst_stride_b % 32 == 0 && dst_stride_h % 32 == 0 && src_stride_b % 8 == 0 && src_stride_h % 8 == 0, "dl_kv_quantize_mx8: strides must keep rows 16-byte aligned");
  DL_REQUIRE((((uintptr_t)k_src | (uintptr_t)v_src | (uintptr_t)k_codes | (uintptr_t)v_codes) & 15) == 0, "dl_kv_quantize_mx8: slabs and code planes must be 16-byte aligned");
  const int64_t items = (int64_t)max_tokens * 2 * (head_dim / 32);
  const dim3 grid((unsigned)((items + 255) / 256), (unsigned)n_kv_heads, (unsigned)B);
  const int e_min = dl_mx8_e_min(model_dtype);
  DL_DISPATCH_DTYPE(src_dtype, T, {
    hipLaunchKernelGGL((kv_quantize_mx8_kernel<T>), grid, dim3(256), 0, as_stream(stream), k_src, v_src, src_stride_b, src_stride_h, src_T_cap,
                       reinterpret_cast<uint8_t*>(k_codes), reinterpret_cast<uint8_t*>(k_scales), reinterpret_cast<uint8_t*>(v_codes), reinterpret_cast<uint8_t*>(v_scales),
                       dst_stride_b, dst_stride_h, dst_T_cap, cu_seqlens, kv_base, head_dim, e_min, err_flag);
  });
  DL_CHECK_LAUNCH("dl_kv_quantize_mx8");
  return DL_OK;
}

extern "C" int dl_attn_decode_rope_kv8(const void* qkv, int64_t qkv_row_stride, const void* cos_tab, const void* sin_tab, int n_pos, const int32_t* pos_base,
                                       const int32_t* kv_len, void* k_codes, void* k_scales, void* v_codes, void* v_scales, int64_t plane_stride_b,
                                       int64_t plane_stride_h, int T_cap, void* out, int64_t out_row_stride, void* workspace, int n_splits, int keys_in_flight,
                                       int chunk_keys, int B, int n_heads, int n_kv_heads, int head_dim, int dtype, void* stream) {
  DL_REQUIRE(keys_in_flight == 128 || keys_in_flight == 256, "dl_attn_decode_rope_kv8: keys_in_flight must be 128 (four waves) or 256 (eight waves)");
  DL_REQUIRE(chunk_keys >= 0, "dl_attn_decode_rope_kv8: chunk_keys must be >= 0");
  DL_REQUIRE(qkv && cos_tab && sin_tab && pos_base && kv_len && out, "dl_attn_decode_rope_kv8: NULL pointer");
  DL_REQUIRE(k_codes && k_scales && v_codes && v_scales, "dl_attn_decode_rope_kv8: NULL plane");
  DL_REQUIRE(head_dim % 32 == 0, "dl_attn_decode_rope_kv8: head_dim=%d is not a multiple of 32 (the scale block)", head_dim);
  DL_REQUIRE(head_dim == 128 || head_dim == 64, "dl_attn_decode_rope_kv8: head_dim=%d unsupported (64 or 128)", head_dim);
  DL_REQUIRE(B > 0 && n_heads > 0 && n_kv_heads > 0 && n_heads % n_kv_heads == 0 && n_pos > 0 && T_cap > 0, "dl_attn_decode_rope_kv8: bad shape");
  DL_REQUIRE(n_splits >= 1 && n_splits <= kMaxSplits, "dl_attn_decode_rope_kv8: n_splits=%d must be in [1, %d]", n_splits, kMaxSplits);
  DL_REQUIRE(n_splits == 1 || workspace, "dl_attn_decode_rope_kv8: workspace required when n_splits > 1");
  DL_REQUIRE(plane_stride_b % 32 == 0 && plane_stride_h % 32 == 0 && (((uintptr_t)k_codes | (uintptr_t)v_codes) & 15) == 0,
             "dl_attn_decode_rope_kv8: code planes must be 16-byte aligned, strides multiples of 32");
  DL_REQUIRE(dtype == DL_F32 || dtype == DL_F16 || dtype == DL_BF16, "dl_attn_decode_rope_kv8: unsupported dtype %d", dtype);
  hipStream_t st = as_stream(stream);
  const int e_min = dl_mx8_e_min(dtype);
#define DL_KV8_ARGS qkv, qkv_row_stride, k_codes, k_scales, v_codes, v_scales, plane_stride_b, plane_stride_h, kv_len, out, out_row_stride, workspace, n_splits, B, n_heads, n_kv_heads, cos_tab, sin_tab, n_pos, pos_base, T_cap, chunk_keys, e_min, st
  // keys_in_flight counts keys at head_dim 128 (a wave-wide load is 8 rows there, 16 at head_dim 64): NW * 8 * U
  DL_DISPATCH_DTYPE(dtype, T, {
    if (head_dim == 128) {
      if (keys_in_flight == 256) launch_kv8<T, 128, 8, 4>(DL_KV8_ARGS);
      else launch_kv8<T, 128, 4, 4>(DL_KV8_ARGS);
    } else {
      if (keys_in_flight == 256) launch_kv8<T, 64, 8, 4>(DL_KV8_ARGS);
      else launch_kv8<T, 64, 4, 4>(DL_KV8_ARGS);
    }
  });
#undef DL_KV8_ARGS
  DL_CHECK_LAUNCH("dl_attn_decode_rope_kv8");
  return DL_OK;
}
