// Device-side log-probabilities of the tokens generate() picks: after the step-closing launch (dl_decode_advance / dl_decode_sample) has committed a row's
// token, this launch reads the step's RAW logits once more and writes the token's log-probability and the n most probable tokens of the step.
// The rule is dynamic_llava_amd/logprobs.py (the contract this kernel is tested against); in short, per row:
//   m, mass_v, M and lse exactly as dl_decode_score (score.hip, scoring.py): M = sum_v floor(expf(x_v - m) * 2^40), lse = logf(float(M) * 2^-40);
//   logprob(v) = -((m - x_v) + lse): the bit-exact negative of dl_decode_score's nll for the label v;
//   the top-n list is the first n entries of the vocabulary ordered by (logit descending, index ascending).
// M is an integer sum: exact, so the same bits however the row is split over threads, waves and launch forms.
//
// One workgroup of 1024 threads per row, the row held as decode_score_kernel holds it (step_close.h: row_chunk, DL_DISPATCH_ROW_REGS): a 16-bit row in
// registers, an fp32 row streamed (read again per pass, from L2).  Pass 1: max / argmax (the owner of the token keeps its logit) = entry 0 of the list;
// pass 2: the masses; then n - 1 selection rounds, round k an argmax over the entries that come AFTER round k - 1's winner in the order above
// (x < prev, or x == prev and v > prev_idx): nothing is removed and no thread keeps state between rounds.  Every loop has a trip count that is uniform
// over the workgroup; no workspace, no global atomics, nothing that synchronises with the host; thread 0 stores the results.
#include "dl_common.h"
#include "fixed_mass.h"
#include "step_close.h"

namespace dl {

constexpr int kMaxTopLogprobs = 8;  // logprobs.py MAX_TOP_LOGPROBS

template <typename T, int R>
__global__ __launch_bounds__(1024) void decode_logprobs_kernel(const void* __restrict__ logits, int64_t row_stride, int V, const int64_t* __restrict__ next_ids,
                                                                const int32_t* __restrict__ step, int cap, float* __restrict__ logprobs, int n_top, int top_stride,
                                                                float* __restrict__ top_logprobs, int64_t* __restrict__ top_ids) {
  constexpr int VE = Elem<T>::kVec;
  constexpr bool kStream = R == 0;  // fp32 logits: nothing is held, every pass reads the thread's chunks
  static_assert(kStream == (VE == 4), "register-resident rows for 16-bit logits, streamed rows for fp32");
  using S = typename Elem<T>::storage;
  __shared__ float s_max[16];
  __shared__ int s_idx[16];
  __shared__ unsigned long long s_sum[16];
  __shared__ float s_xtok;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  // uniform over the workgroup: the slot the step-closing launch has just filled, and its token
  const int slot = step[b] - 1;
  if (slot < 0 || slot >= cap) return;  // (nothing committed yet, or past the buffers: nothing is written)
  const int64_t t64 = next_ids[b];
  const int tok = (t64 >= 0 && t64 < (int64_t)V) ? (int)t64 : -1;  // a token outside [0, V) is never used as an index

  const S* row = reinterpret_cast<const S*>(logits) + (int64_t)b * row_stride;
  const bool vec_ok = (row_stride % VE == 0) && ((reinterpret_cast<uintptr_t>(logits) & 15) == 0);
  const int n_chunks = (V + VE - 1) / VE;  // (the last one may be partial)
  auto fetch = [&](int c) -> uint4 { return row_chunk<T>(row, c * VE, V, vec_ok); };
  auto elem = [](const uint4& q, int e) -> float {
    const uint32_t q4[4] = {q.x, q.y, q.z, q.w};
    if constexpr (VE == 4) return __uint_as_float(q4[e]);
    else return Elem<T>::to_f((S)((q4[e >> 1] >> (16 * (e & 1))) & 0xffffu));
  };
  uint4 raw[kStream ? 1 : R];
  // visit(c, chunk) for each of the thread's chunks c = tid, tid + 1024, ...: the same number of trips in every thread
  auto each_chunk = [&](auto&& visit) {
    if constexpr (kStream) {
      for (int c0 = 0; c0 < n_chunks; c0 += 1024) {
        if (c0 + tid < n_chunks) visit(c0 + tid, fetch(c0 + tid));
      }
    } else {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        visit(r * 1024 + tid, raw[r]);
        __builtin_amdgcn_sched_barrier(0);  // one chunk at a time: interleaving the unrolled bodies only costs registers
      }
    }
  };
  if constexpr (!kStream) {
#pragma unroll
    for (int r = 0; r < R; ++r) raw[r] = fetch(r * 1024 + tid);
  }

  // ---- pass 1: max, argmax (lowest index on ties: dl_decode_advance's rule) and the token's logit ----
  float best = -INFINITY, xt = 0.f;
  int bi = 0x7fffffff, mine = 0;
  each_chunk([&](int c, const uint4& q) {
#pragma unroll
    for (int e = 0; e < VE; ++e) {
      const int v = c * VE + e;
      if (v < V) {
        const float x = elem(q, e);
        argmax_take(best, bi, x, v);
        if (v == tok) {
          xt = x;
          mine = 1;
        }
      }
    }
  });
  if (mine) s_xtok = xt;  // exactly one thread (read after block_argmax's barrier)
  block_argmax(best, bi, s_max, s_idx, lane, wid);
  const float m = best;

  // ---- pass 2: M = sum of floor(expf(x - m) * 2^40), a 64-bit integer sum ----
  uint64_t acc = 0;
  each_chunk([&](int c, const uint4& q) {
#pragma unroll
    for (int e = 0; e < VE; ++e) {
      if (c * VE + e < V) acc += sample_mass(expf(elem(q, e) - m));
    }
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += (uint64_t)__shfl_xor((unsigned long long)acc, o, 64);
  if (lane == 0) s_sum[wid] = (unsigned long long)acc;
  __syncthreads();  // (also: every thread has read pass 1's s_max / s_idx, which the first selection round overwrites)

  const int64_t at = (int64_t)b * cap + slot;
  float lse = 0.f;
  if (tid == 0) {
    uint64_t M = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) M += (uint64_t)s_sum[w];
    lse = logf((float)M * 0x1p-40f);  // u64 -> fp32 rounds to nearest even; the scaling is exact
    logprobs[at] = tok >= 0 ? -((m - s_xtok) + lse) : 0.f;
    if (n_top > 0) {
      top_logprobs[at * top_stride] = -((m - m) + lse);
      top_ids[at * top_stride] = bi;
    }
  }

  // ---- selection rounds: entry k of the list is the argmax over what comes after entry k - 1 ----
  float prev = m;
  int prev_idx = bi;
  for (int k = 1; k < n_top; ++k) {  // (n_top is a launch argument: uniform)
    if (k > 1) __syncthreads();  // the slowest wave has read round k - 1's s_max / s_idx before anybody overwrites them
    best = -INFINITY;
    bi = 0x7fffffff;
    if constexpr (!kStream) {
      // (an empty statement that "rewrites" the row's registers: without it the compiler decodes the whole row to fp32 once in front of the rounds and
      // keeps both forms, which spills at R = 8)
#pragma unroll
      for (int r = 0; r < R; ++r) asm volatile("" : "+v"(raw[r].x), "+v"(raw[r].y), "+v"(raw[r].z), "+v"(raw[r].w));
    }
    each_chunk([&](int c, const uint4& q) {
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        const int v = c * VE + e;
        if (v < V) {
          const float x = elem(q, e);
          if (x < prev || (x == prev && v > prev_idx)) argmax_take(best, bi, x, v);
        }
      }
    });
    block_argmax(best, bi, s_max, s_idx, lane, wid);
    if (tid == 0) {
      top_logprobs[at * top_stride + k] = -((m - best) + lse);
      top_ids[at * top_stride + k] = bi;
    }
    prev = best;
    prev_idx = bi;
  }
}

}  // namespace dl

using namespace dl;

extern "C" int dl_decode_logprobs(const void* logits, int logits_dtype, int64_t logits_row_stride, int V, int B, const int64_t* next_ids, const int32_t* step,
                                  int cap, float* logprobs, int n_top, int top_stride, float* top_logprobs, int64_t* top_ids, void* stream) {
  DL_REQUIRE(logits && next_ids && step && logprobs, "dl_decode_logprobs: NULL pointer");
  DL_REQUIRE(B > 0 && V > 0 && cap > 0, "dl_decode_logprobs: bad shape");
  DL_REQUIRE(V <= kSampleMaxV, "dl_decode_logprobs: V=%d exceeds %d (64-bit fixed-point masses)", V, kSampleMaxV);
  DL_REQUIRE(n_top >= 0 && n_top <= kMaxTopLogprobs, "dl_decode_logprobs: n_top=%d outside 0..%d", n_top, kMaxTopLogprobs);
  DL_REQUIRE(n_top <= V, "dl_decode_logprobs: n_top=%d exceeds V=%d", n_top, V);
  DL_REQUIRE(n_top <= top_stride, "dl_decode_logprobs: n_top=%d exceeds top_stride=%d", n_top, top_stride);
  DL_REQUIRE(n_top == 0 || (top_logprobs && top_ids), "dl_decode_logprobs: n_top=%d without top_logprobs / top_ids", n_top);
  hipStream_t st = as_stream(stream);
  DL_DISPATCH_DTYPE(logits_dtype, T, {
    DL_DISPATCH_ROW_REGS(T, V, R, {
      hipLaunchKernelGGL((decode_logprobs_kernel<T, R>), dim3((unsigned)B), dim3(1024), 0, st, logits, logits_row_stride, V, next_ids, step, cap, logprobs, n_top,
                         top_stride, top_logprobs, top_ids);
    });
  });
  DL_CHECK_LAUNCH("dl_decode_logprobs");
  return DL_OK;
}
