// Classifier-free guidance on paired rows (generate(guidance_scale=, negative_prompt_ids= / negative_images=)): dl_logits_guide in front of the step's other
// logits launches, dl_pair_follow directly behind the step-closing one.  The rule is dynamic_llava_amd/guidance.py (the contract these kernels are tested against).
//
// dl_logits_guide, per pair p (conditional row p, negative row n_pairs + p of the same [2 * n_pairs, V] logits):
//   lc(v) = -((m_c - c_v) + lse_c) and lu(v) = -((m_u - u_v) + lse_u): m, the masses, M and lse exactly as dl_decode_logprobs (logprobs.hip, fixed_mass.h);
//   g(v) = s * (lc - lu) + lu as three rounded fp32 operations (no contraction); -inf where either logit is -inf;
//   with the cutoff on, -inf where lc(v) < (-lse_c) + log_beta;
//   g goes, as fp32, to rows p and n_pairs + p of `out`.  The logits are only read.
// One workgroup of 1024 threads per pair, the rows held as the step-closing kernels hold one (step_close.h: row_chunk, DL_DISPATCH_ROW_REGS): 16-bit rows of up to
// 32768 entries (R = 4) both in registers (108 VGPRs, no scratch); longer 16-bit rows (R = 8) are read again per pass, from L2, as fp32 rows are -- two such
// rows do not fit 128 registers beside the arithmetic (a register-resident build spilled 276-484 bytes per lane).
// Pass 1: the two maxima; pass 2: the two integer masses; pass 3: g.  Every loop has a workgroup-uniform trip count; no
// workspace, no atomics, nothing that synchronises with the host.  Scale, cutoff flag and log_beta are read from device memory (dl_guide_params).
#include "dl_common.h"
#include "fixed_mass.h"
#include "step_close.h"

namespace dl {

template <typename T, int R>
__global__ __launch_bounds__(1024) void logits_guide_kernel(const void* __restrict__ logits, int64_t row_stride, int V, int n_pairs, float* __restrict__ out,
                                                             const dl_guide_params* __restrict__ params) {
  constexpr int VE = Elem<T>::kVec;
  constexpr bool kStream = R == 0;
  static_assert(kStream == (VE == 4), "register-resident rows for 16-bit logits, streamed rows for fp32");
  using S = typename Elem<T>::storage;
  __shared__ float s_mc[16], s_mu[16];
  __shared__ unsigned long long s_sc[16], s_su[16];
  __shared__ float s_lse[2];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const float scale = params->scale;
  const bool cut = params->cutoff_on != 0;
  const float log_beta = params->log_beta;

  const S* row_c = reinterpret_cast<const S*>(logits) + (int64_t)p * row_stride;
  const S* row_u = reinterpret_cast<const S*>(logits) + (int64_t)(n_pairs + p) * row_stride;
  const bool vec_ok = (row_stride % VE == 0) && ((reinterpret_cast<uintptr_t>(logits) & 15) == 0);
  const int n_chunks = (V + VE - 1) / VE;
  auto elem = [](const uint4& q, int e) -> float {
    const uint32_t q4[4] = {q.x, q.y, q.z, q.w};
    if constexpr (VE == 4) return __uint_as_float(q4[e]);
    else return Elem<T>::to_f((S)((q4[e >> 1] >> (16 * (e & 1))) & 0xffffu));
  };
  constexpr bool kHold = !kStream && R <= 4;  // both rows stay in registers
  uint4 raw_c[kHold ? R : 1], raw_u[kHold ? R : 1];
  // visit(c, chunk of the conditional row, chunk of the negative row) for each of the thread's chunks c = tid, tid + 1024, ...
  auto each_chunk = [&](auto&& visit) {
    if constexpr (!kHold) {
      for (int c0 = 0; c0 < n_chunks; c0 += 1024) {
        if (c0 + tid < n_chunks) visit(c0 + tid, row_chunk<T>(row_c, (c0 + tid) * VE, V, vec_ok), row_chunk<T>(row_u, (c0 + tid) * VE, V, vec_ok));
      }
    } else {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        visit(r * 1024 + tid, raw_c[r], raw_u[r]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };
  if constexpr (kHold) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      raw_c[r] = row_chunk<T>(row_c, (r * 1024 + tid) * VE, V, vec_ok);  // (a chunk at or past V is zero bits nobody looks at)
      raw_u[r] = row_chunk<T>(row_u, (r * 1024 + tid) * VE, V, vec_ok);
    }
  }

  // ---- pass 1: the two maxima ----
  float mc = -INFINITY, mu = -INFINITY;
  each_chunk([&](int c, const uint4& qc, const uint4& qu) {
#pragma unroll
    for (int e = 0; e < VE; ++e) {
      if (c * VE + e < V) {
        mc = fmaxf(mc, elem(qc, e));
        mu = fmaxf(mu, elem(qu, e));
      }
    }
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mc = fmaxf(mc, __shfl_xor(mc, o, 64));
    mu = fmaxf(mu, __shfl_xor(mu, o, 64));
  }
  if (lane == 0) {
    s_mc[wid] = mc;
    s_mu[wid] = mu;
  }
  __syncthreads();
  mc = s_mc[0];
  mu = s_mu[0];
#pragma unroll
  for (int w = 1; w < 16; ++w) {
    mc = fmaxf(mc, s_mc[w]);
    mu = fmaxf(mu, s_mu[w]);
  }

  // ---- pass 2: M = sum of floor(expf(x - m) * 2^40) for either row, 64-bit integer sums ----
  if constexpr (kHold) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      asm volatile("" : "+v"(raw_c[r].x), "+v"(raw_c[r].y), "+v"(raw_c[r].z), "+v"(raw_c[r].w));  // (the decoded fp32 form of pass 1 is not kept beside the 16-bit one)
      asm volatile("" : "+v"(raw_u[r].x), "+v"(raw_u[r].y), "+v"(raw_u[r].z), "+v"(raw_u[r].w));
    }
  }
  uint64_t ac = 0, au = 0;
  each_chunk([&](int c, const uint4& qc, const uint4& qu) {
#pragma unroll
    for (int e = 0; e < VE; ++e) {
      if (c * VE + e < V) {
        ac += sample_mass(expf(elem(qc, e) - mc));
        au += sample_mass(expf(elem(qu, e) - mu));
      }
    }
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ac += (uint64_t)__shfl_xor((unsigned long long)ac, o, 64);
    au += (uint64_t)__shfl_xor((unsigned long long)au, o, 64);
  }
  if (lane == 0) {
    s_sc[wid] = (unsigned long long)ac;
    s_su[wid] = (unsigned long long)au;
  }
  __syncthreads();
  if (tid < 2) {
    const unsigned long long* s = tid == 0 ? s_sc : s_su;
    uint64_t M = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) M += (uint64_t)s[w];
    s_lse[tid] = logf((float)M * 0x1p-40f);  // u64 -> fp32 rounds to nearest even; the scaling is exact
  }
  __syncthreads();
  const float lse_c = s_lse[0], lse_u = s_lse[1];
  const float thr = __fadd_rn(-lse_c, log_beta);  // the conditional maximum's log-probability is -((m - m) + lse) = -lse

  // ---- pass 3: g, to both rows of the pair ----
  float* out_c = out + (int64_t)p * V;
  float* out_u = out + (int64_t)(n_pairs + p) * V;
  const bool st_vec = (V % 4 == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
  if constexpr (kHold) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      asm volatile("" : "+v"(raw_c[r].x), "+v"(raw_c[r].y), "+v"(raw_c[r].z), "+v"(raw_c[r].w));  // (keeps the rows in their 16-bit form: see logprobs.hip)
      asm volatile("" : "+v"(raw_u[r].x), "+v"(raw_u[r].y), "+v"(raw_u[r].z), "+v"(raw_u[r].w));
    }
  }
  each_chunk([&](int c, const uint4& qc, const uint4& qu) {
    float g[VE];
#pragma unroll
    for (int e = 0; e < VE; ++e) {
      const float xc = elem(qc, e), xu = elem(qu, e);
      const float lc = -__fadd_rn(__fsub_rn(mc, xc), lse_c);
      const float lu = -__fadd_rn(__fsub_rn(mu, xu), lse_u);
      float v = __fadd_rn(__fmul_rn(scale, __fsub_rn(lc, lu)), lu);
      if (xc == -INFINITY || xu == -INFINITY) v = -INFINITY;
      if (cut && !(lc >= thr)) v = -INFINITY;
      g[e] = v;
    }
    const int v0 = c * VE;
    if (v0 >= V) return;  // (a register chunk past the row)
    if (st_vec && v0 + VE <= V) {
#pragma unroll
      for (int q = 0; q < VE / 4; ++q) {
        const float4 w = make_float4(g[4 * q], g[4 * q + 1], g[4 * q + 2], g[4 * q + 3]);
        *reinterpret_cast<float4*>(out_c + v0 + 4 * q) = w;
        *reinterpret_cast<float4*>(out_u + v0 + 4 * q) = w;
      }
    } else {
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        if (v0 + e < V) {
          out_c[v0 + e] = g[e];
          out_u[v0 + e] = g[e];
        }
      }
    }
  });
}

// One thread per pair: the negative row takes the conditional row's token, its out_ids slot and its finished flag.
__global__ __launch_bounds__(256) void pair_follow_kernel(int n_pairs, int64_t* __restrict__ next_ids, int64_t* __restrict__ out_ids, int out_cap,
                                                          const int32_t* __restrict__ step, int32_t* __restrict__ finished) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n_pairs) return;
  const int n = n_pairs + b;
  next_ids[n] = next_ids[b];
  const int slot = step[b] - 1;  // the slot the step-closing launch has just filled
  if (slot >= 0 && slot < out_cap) out_ids[(int64_t)n * out_cap + slot] = out_ids[(int64_t)b * out_cap + slot];
  finished[n] = finished[b];
}

}  // namespace dl

using namespace dl;

extern "C" int dl_logits_guide(const void* logits, int logits_dtype, int64_t logits_row_stride, int V, int n_pairs, float* out, const dl_guide_params* params,
                               void* stream) {
  DL_REQUIRE(logits && out && params, "dl_logits_guide: NULL pointer");
  DL_REQUIRE(n_pairs > 0 && V > 0, "dl_logits_guide: bad shape (n_pairs=%d V=%d)", n_pairs, V);
  DL_REQUIRE(V <= kSampleMaxV, "dl_logits_guide: V=%d exceeds %d (64-bit fixed-point masses)", V, kSampleMaxV);
  DL_REQUIRE(n_pairs <= 32767, "dl_logits_guide: n_pairs=%d exceeds 32767", n_pairs);
  DL_REQUIRE(logits_row_stride >= V, "dl_logits_guide: row stride %lld below V=%d", (long long)logits_row_stride, V);
  DL_REQUIRE((const void*)out != logits, "dl_logits_guide: out must not be the logits");
  hipStream_t st = as_stream(stream);
  DL_DISPATCH_DTYPE(logits_dtype, T, {
    DL_DISPATCH_ROW_REGS(T, V, R, {
      hipLaunchKernelGGL((logits_guide_kernel<T, R>), dim3((unsigned)n_pairs), dim3(1024), 0, st, logits, logits_row_stride, V, n_pairs, out, params);
    });
  });
  DL_CHECK_LAUNCH("dl_logits_guide");
  return DL_OK;
}

extern "C" int dl_pair_follow(int n_pairs, int64_t* next_ids, int64_t* out_ids, int out_cap, const int32_t* step, int32_t* finished, void* stream) {
  DL_REQUIRE(next_ids && out_ids && step && finished, "dl_pair_follow: NULL pointer");
  DL_REQUIRE(n_pairs >= 1 && out_cap >= 1, "dl_pair_follow: bad shape n_pairs=%d out_cap=%d", n_pairs, out_cap);
  hipLaunchKernelGGL(pair_follow_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, as_stream(stream), n_pairs, next_ids, out_ids, out_cap, step, finished);
  DL_CHECK_LAUNCH("dl_pair_follow");
  return DL_OK;
}
