// The rule that closes a decode step, shared by the three kernels that can end one: dl_decode_advance (argmax), dl_decode_sample (a drawn token) and
// dl_decode_score (the label).  Each picks the row's next token its own way; what happens to the token afterwards is written here once.
#pragma once
#include "dl_common.h"

namespace dl {

// The EOS set: up to three ids.  eos_set() is the one place that normalises it: without a first id there is no set, and unused ids are -1 (no
// vocabulary index is negative, so they never compare equal to a token).
struct EosSet {
  int id, id2, id3;
  __device__ __forceinline__ bool has(int v) const { return v == id || v == id2 || v == id3; }
};
constexpr EosSet kNoEos = {-1, -1, -1};
constexpr EosSet eos_set(int eos_id, int eos_id2, int eos_id3) { return eos_id >= 0 ? EosSet{eos_id, eos_id2, eos_id3} : kNoEos; }

// HF MinNewTokensLengthLogitsProcessor: the EOS logits are -inf while fewer than min_new_tokens tokens exist.  -> the ids that are out of this step's
// selection (uniform per row)
__device__ __forceinline__ EosSet banned_ids(const EosSet& eos, int min_new_tokens, int cur_step) {
  return eos.id >= 0 && min_new_tokens > 0 && cur_step < min_new_tokens ? eos : kNoEos;
}

// What a step-closing launch updates, per row b (a NULL pointer: that part of the state is not kept).
struct StepClose {
  int64_t *next_ids, *out_ids;  // out_ids [B, out_cap]: slot step[b] takes the token while there is one
  int out_cap;
  int32_t *step, *finished;
  int pad_id;
  int32_t *kv_len_full, *kv_len_sparse;
  const int32_t* decision;  // the text predictor's keep (1) / evict (0)
};

// The row's state as thread 0 finds it.  preload() goes in front of the row's reduction, so that these loads are in flight while the logits are read.
// with_finished = false: a caller whose pick for a finished row is pad_id already leaves that flag alone.
struct StepRow {
  int fin = 0, step = 0, dec = 1, full = 0, sparse = 0;
  __device__ __forceinline__ void preload(const StepClose& c, int b, bool with_finished = true) {
    if (with_finished && c.finished) fin = c.finished[b];
    if (c.step) step = c.step[b];
    if (c.decision) dec = c.decision[b];
    if (c.kv_len_full) full = c.kv_len_full[b];
    if (c.kv_len_sparse) sparse = c.kv_len_sparse[b];
  }
  // tok is the row's pick: a finished row emits pad_id instead, a token of the EOS set finishes the row; the token is appended while out_ids has room,
  // the step counter advances either way, and the KV lengths advance by 1 and by the predictor's decision.  (One thread per row.)
  __device__ __forceinline__ void commit(int tok, const StepClose& c, const EosSet& eos, int b) const {
    if (c.finished) {
      if (fin) tok = c.pad_id;
      else if (eos.id >= 0 && eos.has(tok)) c.finished[b] = 1;
    }
    c.next_ids[b] = tok;
    if (c.out_ids && c.step) {
      if (step < c.out_cap) c.out_ids[(int64_t)b * c.out_cap + step] = tok;
      c.step[b] = step + 1;
    }
    if (c.kv_len_full) c.kv_len_full[b] = full + 1;
    if (c.kv_len_sparse) c.kv_len_sparse[b] = sparse + dec;
  }
};

// (best, bi) takes (ob, oi) if that is the larger value, or the same value at a lower index
__device__ __forceinline__ void argmax_take(float& best, int& bi, float ob, int oi) {
  if (ob > best || (ob == best && oi < bi)) {
    best = ob;
    bi = oi;
  }
}

// Argmax over a workgroup of 16 waves, the lowest index winning ties: each thread brings its own (best, bi) -- (-inf, 0x7fffffff) when it saw nothing --
// and every thread leaves with the block's.  smax / sidx: 16 LDS slots each.  Contains the workgroup's barrier.
__device__ __forceinline__ void block_argmax(float& best, int& bi, float* smax, int* sidx, int lane, int wid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) argmax_take(best, bi, __shfl_xor(best, o, 64), __shfl_xor(bi, o, 64));
  if (lane == 0) {
    smax[wid] = best;
    sidx[wid] = bi;
  }
  __syncthreads();
  best = smax[0];
  bi = sidx[0];
#pragma unroll
  for (int w = 1; w < 16; ++w) argmax_take(best, bi, smax[w], sidx[w]);
  if (bi == 0x7fffffff) bi = 0;
}

// The 16 bytes of a row that start at entry v0 (a multiple of the chunk's VE entries).  A row that is not 16-byte addressable (vec_ok false), and the partial
// last chunk of any row, take scalar loads into the same registers; entries at or past V are zero bits that nobody looks at.
template <typename T>
__device__ __forceinline__ uint4 row_chunk(const typename Elem<T>::storage* row, int v0, int V, bool vec_ok) {
  constexpr int VE = Elem<T>::kVec;
  if (vec_ok && v0 + VE <= V) return *reinterpret_cast<const uint4*>(row + v0);
  uint32_t t4[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int e = 0; e < VE; ++e) {
    if (v0 + e < V) {
      if constexpr (VE == 4) t4[e] = __float_as_uint((float)row[v0 + e]);
      else t4[e >> 1] |= (uint32_t)row[v0 + e] << (16 * (e & 1));
    }
  }
  return make_uint4(t4[0], t4[1], t4[2], t4[3]);
}

// Rows held in registers: R 16-byte chunks per thread of a 1024-thread workgroup for 16-bit logits (4 up to 32768 entries, 8 up to 65536); R = 0 streams an
// fp32 row instead.  Runs the body with R a constant.
#define DL_DISPATCH_ROW_REGS(T, V, R, ...)                               \
  if constexpr (Elem<T>::kVec != 8) { constexpr int R = 0; __VA_ARGS__ } \
  else if ((V) <= 1024 * 4 * 8) { constexpr int R = 4; __VA_ARGS__ }     \
  else { constexpr int R = 8; __VA_ARGS__ }

}  // namespace dl
