// Device-side logits processors: repetition penalty, no-repeat n-gram and bad-word bans of one decode step, the stage HF's generate() runs in front of
// the selection rule (RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor, NoBadWordsLogitsProcessor, in that order).  It sits between the
// lm_head launch and the bookkeeping launch (dl_decode_advance in advance.hip / dl_decode_sample in sample.hip), which consume its fp32 output unchanged.
// The rule is dynamic_llava_amd/logits_rules.py (the contract this kernel is tested against); in short, per row, with g = the row's tokens emitted so
// far (out_ids[b, 0 : min(step[b], out_cap)]) and s = len(g):
//   y_v = float32(logit_v);
//   penalty p (> 0, != 1): every t in g gets y_t = x_t < 0 ? x_t * p : x_t / p -- ONE fp32 operation on the input logit (IEEE division);
//   n-gram n (>= 1, s + 1 >= n): every i in [0, s - n] with g[i : i + n - 1] == the last n - 1 tokens of g bans g[i + n - 1];
//   bad words: a one-token word bans its id; a longer one bans its last id when len <= s and the last len - 1 tokens of g equal the ids in front of it;
//   a banned id is -inf, whatever the penalty made of it.
//
// One workgroup of 256 threads owns kTile consecutive entries of one row.  It converts them (one 16-byte load per thread where the row is 16-byte
// addressable, scalar loads for odd strides and for the last entries of a row), then, after a workgroup barrier, writes the penalty edits that fall
// inside its range, and after a second barrier the bans.  Every edit is computed from the INPUT logit, never from `out`: a token that occurs many
// times in the history gets the same value from every writer, so nothing is de-duplicated, nothing is atomic and there is no workspace.  Every
// workgroup of a row scans the row's whole history itself (at most out_cap ids).  An id outside the workgroup's range -- in particular one outside
// [0, V) -- is never used as an index.  Nothing synchronises with the host.
#include "dl_common.h"

namespace dl {

constexpr int kLpThreads = 256;
constexpr int kLpPerThread = 8;  // one 16-byte load of a 16-bit row, two of an fp32 row
constexpr int kLpTile = kLpThreads * kLpPerThread;

struct dl_logits_params_dev {  // == dl_logits_params (include/dynllava.h)
  float repetition_penalty;
  int32_t no_repeat_ngram;
  int32_t n_bad_words;
  int32_t reserved[5];
};

template <typename T>
__global__ __launch_bounds__(kLpThreads) void logits_process_kernel(const void* __restrict__ logits, int64_t row_stride, int V, float* __restrict__ out,
                                                                      const int64_t* __restrict__ out_ids, int out_cap, const int32_t* __restrict__ step,
                                                                      const dl_logits_params_dev* __restrict__ prm, const int32_t* __restrict__ bad_words) {
  constexpr int VE = Elem<T>::kVec;
  using S = typename Elem<T>::storage;
  const int b = blockIdx.y, tid = threadIdx.x;
  const int lo = blockIdx.x * kLpTile;
  const int hi = lo + kLpTile < V ? lo + kLpTile : V;  // this workgroup's range [lo, hi)
  const S* row = reinterpret_cast<const S*>(logits) + (int64_t)b * row_stride;
  float* orow = out + (int64_t)b * V;

  // ---- convert the range ----
  const bool in_vec = (row_stride % VE == 0) && ((reinterpret_cast<uintptr_t>(logits) & 15) == 0);
  const bool out_vec = (V % 4 == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
  const int v0 = lo + tid * kLpPerThread;
  if (v0 + kLpPerThread <= V) {
    float f[kLpPerThread];
    if (in_vec) {
#pragma unroll
      for (int c = 0; c < kLpPerThread / VE; ++c) {
        float t[VE];
        load16<T>(row + v0 + c * VE, t);
#pragma unroll
        for (int e = 0; e < VE; ++e) f[c * VE + e] = t[e];
      }
    } else {
#pragma unroll
      for (int e = 0; e < kLpPerThread; ++e) f[e] = Elem<T>::to_f(row[v0 + e]);
    }
    if (out_vec) {
      *reinterpret_cast<float4*>(orow + v0) = make_float4(f[0], f[1], f[2], f[3]);
      *reinterpret_cast<float4*>(orow + v0 + 4) = make_float4(f[4], f[5], f[6], f[7]);
    } else {
#pragma unroll
      for (int e = 0; e < kLpPerThread; ++e) orow[v0 + e] = f[e];
    }
  } else {
    for (int v = v0; v < V; ++v) orow[v] = Elem<T>::to_f(row[v]);  // the row's last, partial group (v0 >= V: nothing)
  }

  // ---- the row's history: uniform over the workgroup ----
  int s = 0;
  if (step && out_ids) {
    s = step[b];
    s = s < 0 ? 0 : (s > out_cap ? out_cap : s);
  }
  const int64_t* g = s > 0 ? out_ids + (int64_t)b * out_cap : nullptr;  // (never read when s == 0)
  const float p = prm->repetition_penalty;
  const int n = prm->no_repeat_ngram;
  int nb = bad_words ? prm->n_bad_words : 0;
  nb = nb < 0 ? 0 : (nb > DL_LOGITS_MAX_BAD_WORDS ? DL_LOGITS_MAX_BAD_WORDS : nb);

  __syncthreads();
  // ---- penalty: one fp32 operation on the input logit; every occurrence of a token writes the same value ----
  if (p > 0.f && p != 1.f) {
    for (int i = tid; i < s; i += kLpThreads) {
      const int64_t t = g[i];
      if (t >= lo && t < hi) {
        const float x = Elem<T>::to_f(row[t]);
        orow[t] = x < 0.f ? x * p : x / p;
      }
    }
  }
  __syncthreads();
  // ---- bans win: written after every penalty write of this range ----
  if (n >= 1 && s + 1 >= n) {
    const int64_t* pre = g + (s - (n - 1));  // the last n - 1 tokens
    for (int i = tid; i <= s - n; i += kLpThreads) {
      bool same = true;
      for (int k = 0; k < n - 1; ++k) same = same && g[i + k] == pre[k];
      const int64_t t = g[i + n - 1];
      if (same && t >= lo && t < hi) orow[t] = -INFINITY;
    }
  }
  for (int w = tid; w < nb; w += kLpThreads) {
    const int32_t* e = bad_words + w * (1 + DL_LOGITS_MAX_BAD_WORD_LEN);
    const int len = e[0];
    if (len < 1 || len > DL_LOGITS_MAX_BAD_WORD_LEN || (len > 1 && len > s)) continue;  // (HF skips a word longer than the history)
    bool same = true;
    for (int k = 0; k < len - 1; ++k) same = same && g[s - (len - 1) + k] == (int64_t)e[1 + k];
    const int t = e[len];
    if (same && t >= lo && t < hi) orow[t] = -INFINITY;
  }
}

}  // namespace dl

using namespace dl;

static_assert(sizeof(dl_logits_params) == sizeof(dl_logits_params_dev) && sizeof(dl_logits_params) == 32, "dl_logits_params layout");

extern "C" int dl_logits_process(const void* logits, int logits_dtype, int64_t logits_row_stride, int V, int B, float* out, const int64_t* out_ids,
                                 int out_cap, const int32_t* step, const dl_logits_params* params, const int32_t* bad_words, void* stream) {
  DL_REQUIRE(logits && out, "dl_logits_process: NULL pointer");
  DL_REQUIRE(params, "dl_logits_process: NULL parameter block");
  DL_REQUIRE(B > 0 && V > 0 && out_cap >= 0, "dl_logits_process: bad shape");
  DL_REQUIRE(B <= 65535, "dl_logits_process: B=%d exceeds 65535 rows", B);
  hipStream_t st = as_stream(stream);
  const dl_logits_params_dev* prm = reinterpret_cast<const dl_logits_params_dev*>(params);
  const dim3 grid((unsigned)((V + kLpTile - 1) / kLpTile), (unsigned)B);
  DL_DISPATCH_DTYPE(logits_dtype, T, {
    hipLaunchKernelGGL((logits_process_kernel<T>), grid, dim3(kLpThreads), 0, st, logits, logits_row_stride, V, out, out_ids, out_cap, step, prm, bad_words);
  });
  DL_CHECK_LAUNCH("dl_logits_process");
  return DL_OK;
}
