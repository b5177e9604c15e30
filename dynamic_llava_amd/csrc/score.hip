// Device-side teacher-forced scoring: the negative log-likelihood of one labelled token per row; the step is closed like dl_decode_advance's
// (advance.hip) by step_close.h, around the LABEL as the next token (the reference's perplexity driver, model_lvis_for_ppl.py:136-191: score the label, feed the label).
// The rule is dynamic_llava_amd/scoring.py (the contract this kernel is tested against); in short, per row:
//   m = max_v x_v (fp32), top1 = lowest index attaining it; mass_v = floor(expf(x_v - m) * 2^40) as a 64-bit integer; M = sum_v mass_v;
//   lse = logf(float(M) * 2^-40); nll = (m - x_label) + lse.
// M is an integer sum: exact, so the same bits however the row is split over threads, waves and launch forms.
//
// One workgroup of 1024 threads per row.  Thread t owns the 16-byte chunks t, t + 1024, ...  A 16-bit row is read once (R chunks per thread, kept in
// registers: R = 4 up to 32768 entries, 8 up to 65536); an fp32 row (the model's step buffer is 16-bit: fp32 is the small-model / test route) is read
// twice, the second time from L2.  A row that is not 16-byte addressable, and the partial last chunk of any row, take scalar loads into the same
// registers: the arithmetic never knows.  Pass 1: max / argmax (and the owner of `label` keeps x_label); pass 2: masses and a 64-bit wave / LDS
// reduction.  Every loop has a fixed trip count; no workspace, no global atomics, nothing that synchronises with the host.
#include "dl_common.h"
#include "fixed_mass.h"
#include "step_close.h"

namespace dl {

template <typename T, int R>
__global__ __launch_bounds__(1024) void decode_score_kernel(const void* __restrict__ logits, int64_t row_stride, int V, const int64_t* __restrict__ labels,
                                                             int label_cap, float* __restrict__ nll, int64_t* __restrict__ top1,
                                                             int64_t* __restrict__ next_ids, int64_t* __restrict__ out_ids, int out_cap,
                                                             int32_t* __restrict__ step, int32_t* __restrict__ finished, int pad_id,
                                                             int32_t* __restrict__ kv_len_full, int32_t* __restrict__ kv_len_sparse,
                                                             const int32_t* __restrict__ decision) {
  constexpr int VE = Elem<T>::kVec;
  constexpr bool kStream = R == 0;  // fp32 logits: nothing is held, both passes read the thread's chunks
  static_assert(kStream == (VE == 4), "register-resident rows for 16-bit logits, streamed rows for fp32");
  using S = typename Elem<T>::storage;
  __shared__ float s_max[16];
  __shared__ int s_idx[16];
  __shared__ unsigned long long s_sum[16];
  __shared__ float s_xlab;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const StepClose sc = {next_ids, out_ids, out_cap, step, finished, pad_id, kv_len_full, kv_len_sparse, decision};
  StepRow st;
  if (tid == 0) st.preload(sc, b, false);  // (a finished row has no label: its pick is pad_id already)
  // uniform over the workgroup: the slot and its label.  A label outside [0, V) is never used as an index: it means "no label".
  const int cur_step = sc.step ? sc.step[b] : 0;
  const int row_done = sc.finished ? sc.finished[b] : 0;
  int lab = -1;
  if (!row_done && cur_step >= 0 && cur_step < label_cap) {
    const int64_t l = labels[(int64_t)b * label_cap + cur_step];
    if (l >= 0 && l < (int64_t)V) lab = (int)l;
  }
  const bool have = lab >= 0;
  float m = 0.f;
  int bi = 0;
  if (have) {
    const S* row = reinterpret_cast<const S*>(logits) + (int64_t)b * row_stride;
    const bool vec_ok = (row_stride % VE == 0) && ((reinterpret_cast<uintptr_t>(logits) & 15) == 0);
    const int n_chunks = (V + VE - 1) / VE;  // (the last one may be partial)
    auto fetch = [&](int c) -> uint4 { return row_chunk<T>(row, c * VE, V, vec_ok); };
    auto elem = [](const uint4& q, int e) -> float {
      const uint32_t q4[4] = {q.x, q.y, q.z, q.w};
      if constexpr (VE == 4) return __uint_as_float(q4[e]);
      else return Elem<T>::to_f((S)((q4[e >> 1] >> (16 * (e & 1))) & 0xffffu));
    };

    // ---- pass 1: max, argmax (lowest index on ties: dl_decode_advance's rule) and the label's logit ----
    float best = -INFINITY, xl = 0.f;
    int mine = 0;
    bi = 0x7fffffff;
    auto visit1 = [&](int c, const uint4& q) {
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        const int v = c * VE + e;
        if (v < V) {
          const float x = elem(q, e);
          if (x > best || (x == best && v < bi)) {
            best = x;
            bi = v;
          }
          if (v == lab) {
            xl = x;
            mine = 1;
          }
        }
      }
    };
    uint4 raw[kStream ? 1 : R];
    if constexpr (kStream) {
      for (int c = tid; c < n_chunks; c += 1024) visit1(c, fetch(c));
    } else {
#pragma unroll
      for (int r = 0; r < R; ++r) raw[r] = fetch(r * 1024 + tid);
#pragma unroll
      for (int r = 0; r < R; ++r) visit1(r * 1024 + tid, raw[r]);
    }
    if (mine) s_xlab = xl;  // exactly one thread (read after block_argmax's barrier)
    block_argmax(best, bi, s_max, s_idx, lane, wid);
    m = best;

    // ---- pass 2: M = sum of floor(expf(x - m) * 2^40), a 64-bit integer sum ----
    uint64_t acc = 0;
    auto visit2 = [&](int c, const uint4& q) {
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        if (c * VE + e < V) acc += sample_mass(expf(elem(q, e) - m));
      }
    };
    if constexpr (kStream) {
      for (int c = tid; c < n_chunks; c += 1024) visit2(c, fetch(c));
    } else {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        visit2(r * 1024 + tid, raw[r]);
        __builtin_amdgcn_sched_barrier(0);  // one chunk at a time: interleaving the unrolled bodies only costs registers
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += (uint64_t)__shfl_xor((unsigned long long)acc, o, 64);
    if (lane == 0) s_sum[wid] = (unsigned long long)acc;
  }
  __syncthreads();
  if (tid == 0) {  // the closing around the label (no EOS set: the label sequence ends the row)
    int tok = sc.pad_id;
    if (have) {
      uint64_t M = 0;
#pragma unroll
      for (int w = 0; w < 16; ++w) M += (uint64_t)s_sum[w];
      const float lse = logf((float)M * 0x1p-40f);  // u64 -> fp32 rounds to nearest even; the scaling is exact
      const float d = m - s_xlab;
      nll[(int64_t)b * label_cap + cur_step] = d + lse;
      if (top1) top1[(int64_t)b * label_cap + cur_step] = bi;
      tok = lab;
    } else if (sc.finished) {
      sc.finished[b] = 1;  // labels exhausted: the scorer's own rule, in front of the shared one
    }
    st.commit(tok, sc, kNoEos, b);
  }
}

}  // namespace dl

using namespace dl;

extern "C" int dl_decode_score(const void* logits, int logits_dtype, int64_t logits_row_stride, int V, int B, const int64_t* labels, int label_cap,
                               float* nll, int64_t* top1, int64_t* next_ids, int64_t* out_ids, int out_cap, int32_t* step, int32_t* finished,
                               int pad_id, int32_t* kv_len_full, int32_t* kv_len_sparse, const int32_t* decision, void* stream) {
  DL_REQUIRE(logits && next_ids, "dl_decode_score: NULL pointer");
  DL_REQUIRE(labels && nll, "dl_decode_score: NULL labels / nll");
  DL_REQUIRE(B > 0 && V > 0 && label_cap > 0 && out_cap >= 0, "dl_decode_score: bad shape");
  DL_REQUIRE(V <= kSampleMaxV, "dl_decode_score: V=%d exceeds %d (64-bit fixed-point masses)", V, kSampleMaxV);
  hipStream_t st = as_stream(stream);
  DL_DISPATCH_DTYPE(logits_dtype, T, {
    DL_DISPATCH_ROW_REGS(T, V, R, {
      hipLaunchKernelGGL((decode_score_kernel<T, R>), dim3((unsigned)B), dim3(1024), 0, st, logits, logits_row_stride, V, labels, label_cap, nll, top1,
                         next_ids, out_ids, out_cap, step, finished, pad_id, kv_len_full, kv_len_sparse, decision);
    });
  });
  DL_CHECK_LAUNCH("dl_decode_score");
  return DL_OK;
}
