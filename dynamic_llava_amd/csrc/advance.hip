// Greedy decode step closing: argmax + the device-side bookkeeping of step_close.h (token append, EOS flags, KV length advance: replaces CU:153-164's
// host sync).  dl_decode_sample (sample.hip) and dl_decode_score (score.hip) close a step the same way around another token.
#include "dl_common.h"
#include "step_close.h"

namespace dl {

// grid (B).  The row (V logits) is read with 16-byte loads, 4 per thread in flight (one round trip for V <= 32768), and thread 0 requests the per-row
// state it will update before the reduction
template <typename T>
__global__ __launch_bounds__(1024) void decode_advance_kernel(const void* __restrict__ logits, int64_t row_stride, int V,
                                                               int64_t* __restrict__ next_ids, int64_t* __restrict__ out_ids, int out_cap,
                                                               int32_t* __restrict__ step, int32_t* __restrict__ finished, EosSet eos, int pad_id,
                                                               int32_t* __restrict__ kv_len_full, int32_t* __restrict__ kv_len_sparse,
                                                               const int32_t* __restrict__ decision, int min_new_tokens) {
  constexpr int VE = Elem<T>::kVec;
  using S = typename Elem<T>::storage;
  __shared__ float smax[16];
  __shared__ int sidx[16];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const StepClose sc = {next_ids, out_ids, out_cap, step, finished, pad_id, kv_len_full, kv_len_sparse, decision};
  StepRow st;
  if (tid == 0) st.preload(sc, b);
  const S* row = reinterpret_cast<const S*>(logits) + (int64_t)b * row_stride;
  const bool vec_ok = (row_stride % VE == 0) && ((reinterpret_cast<uintptr_t>(logits) & 15) == 0);
  const EosSet banned = banned_ids(eos, min_new_tokens, sc.step ? sc.step[b] : 0);
  float best = -INFINITY;
  int bi = 0x7fffffff;
  const int n_chunks = V / VE;
  if (vec_ok) {
    for (int c0 = 0; c0 < n_chunks; c0 += 4 * 1024) {
      float x[4][VE];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int c = c0 + u * 1024 + tid;
        if (c < n_chunks) load16<T>(row + (int64_t)c * VE, x[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int c = c0 + u * 1024 + tid;
        if (c < n_chunks)
#pragma unroll
          for (int e = 0; e < VE; ++e) {
            const int v = c * VE + e;
            if (banned.has(v)) continue;
            if (x[u][e] > best || (x[u][e] == best && v < bi)) {
              best = x[u][e];
              bi = v;
            }
          }
      }
    }
  }
  for (int v = (vec_ok ? n_chunks * VE : 0) + tid; v < V; v += 1024) {  // tail (or the whole row when it is not 16-byte addressable)
    const float xv = load1<T>(logits, (int64_t)b * row_stride + v);
    if (banned.has(v)) continue;
    if (xv > best || (xv == best && v < bi)) {
      best = xv;
      bi = v;
    }
  }
  block_argmax(best, bi, smax, sidx, lane, wid);
  if (tid == 0) st.commit(bi, sc, eos, b);
}

}  // namespace dl

using namespace dl;

extern "C" int dl_decode_advance(const void* logits, int logits_dtype, int64_t logits_row_stride, int V, int B, int64_t* next_ids,
                                 int64_t* out_ids, int out_cap, int32_t* step, int32_t* finished, int eos_id, int eos_id2, int eos_id3, int pad_id,
                                 int32_t* kv_len_full, int32_t* kv_len_sparse, const int32_t* decision, int min_new_tokens,
                                 void* stream) {
  DL_REQUIRE(logits && next_ids, "dl_decode_advance: NULL pointer");
  DL_REQUIRE(B > 0 && V > 0, "dl_decode_advance: bad shape");
  hipStream_t st = as_stream(stream);
  DL_DISPATCH_DTYPE(logits_dtype, T, {
    hipLaunchKernelGGL((decode_advance_kernel<T>), dim3((unsigned)B), dim3(1024), 0, st, logits, logits_row_stride, V, next_ids, out_ids,
                       out_cap, step, finished, eos_set(eos_id, eos_id2, eos_id3), pad_id, kv_len_full, kv_len_sparse, decision, min_new_tokens);
  });
  DL_CHECK_LAUNCH("dl_decode_advance");
  return DL_OK;
}
