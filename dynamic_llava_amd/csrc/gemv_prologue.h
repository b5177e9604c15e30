// The prologues of the weight-streaming GEMVs (gemv.hip on model-dtype rows, gemv_pk.hip on 12-bit packed bf16 rows): ONE copy, so that the
// x a packed launch multiplies with is bit-identical to the x of the launch it replaces.
#pragma once
#include "gemv_dot.h"

namespace dl {

constexpr int kGemvThreads = 256;

// Builds x [B][K] (model dtype) in LDS `xs`.  MODE: 0 plain (copy x), 1 add + rmsnorm (h_out written by workgroup `bid` == 0 when delta is given),
// 2 silu(g) * u of x_ = gate|up [B, 2K].  `red`: four floats of LDS for the block reduction.  The caller synchronises the workgroup afterwards.
template <typename T, int B, int MODE>
__device__ __forceinline__ void gemv_build_x(typename Elem<T>::storage* xs, float* red, int K, const void* x_, int64_t x_rs, const void* __restrict__ h_,
                                             void* __restrict__ h_out_, const void* __restrict__ delta_, const void* __restrict__ nw_, float eps, const int bid) {
  constexpr int V = Elem<T>::kVec;
  using S = typename Elem<T>::storage;
  const int tid = threadIdx.x;
  const int nvec = K / V;
  if constexpr (MODE == 1) {  // ADDNORM
    const S* h = reinterpret_cast<const S*>(h_);
    S* h_out = reinterpret_cast<S*>(h_out_);
    const S* dl_ = reinterpret_cast<const S*>(delta_);
    const S* nw = reinterpret_cast<const S*>(nw_);
    constexpr int MAXC = 4;  // 16-byte chunks per thread held in registers: K <= 256 * 4 * kVec (8192 for the 16-bit dtypes)
    if (nvec <= kGemvThreads * MAXC) {
      // every global load of the prologue (residual row, delta row, norm weight) is requested before anything is used: the
      // prologue is then ONE L2 round trip + the reduction, instead of load -> reduce -> load
      uint4 wr[MAXC];
#pragma unroll
      for (int c = 0; c < MAXC; ++c) {
        const int v = tid + c * kGemvThreads;
        if (v < nvec) wr[c] = *reinterpret_cast<const uint4*>(nw + v * V);
      }
#pragma unroll
      for (int b = 0; b < B; ++b) {
        uint4 hr[MAXC], dr[MAXC];
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
          const int v = tid + c * kGemvThreads;
          if (v < nvec) {
            hr[c] = *reinterpret_cast<const uint4*>(h + (int64_t)b * K + v * V);
            if (dl_) dr[c] = *reinterpret_cast<const uint4*>(dl_ + (int64_t)b * K + v * V);
          }
        }
        float a[MAXC][V];
        float ss = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
          const int v = tid + c * kGemvThreads;
          if (v < nvec) {
            unpack16<T>(hr[c], a[c]);
            if (dl_) {
              float d[V];
              unpack16<T>(dr[c], d);
#pragma unroll
              for (int e = 0; e < V; ++e) a[c][e] = Elem<T>::round(a[c][e] + d[e]);
              // updated residual stream: written once, to a DIFFERENT buffer (other workgroups are still reading h_in)
              if (bid == 0) store16<T>(h_out + (int64_t)b * K + v * V, a[c]);
            }
#pragma unroll
            for (int e = 0; e < V; ++e) ss += a[c][e] * a[c][e];
          }
        }
        const float rstd = rsqrtf(block_sum<4>(ss, red) / (float)K + eps);
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
          const int v = tid + c * kGemvThreads;
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
        for (int v = tid; v < nvec; v += kGemvThreads) {
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
        for (int v = tid; v < nvec; v += kGemvThreads) {
          float a[V], w[V];
          load16<T>(xs + b * K + v * V, a);
          load16<T>(nw + v * V, w);
#pragma unroll
          for (int e = 0; e < V; ++e) a[e] = w[e] * Elem<T>::round(a[e] * rstd);
          store16<T>(xs + b * K + v * V, a);
        }
      }
    }
  } else if constexpr (MODE == 2) {  // SILUMUL: x_ = gate_up [B, 2K]
    const S* gu = reinterpret_cast<const S*>(x_);
#pragma unroll
    for (int b = 0; b < B; ++b)
      for (int v = tid; v < nvec; v += kGemvThreads) {
        float g[V], u[V];
        load16<T>(gu + (int64_t)b * x_rs + v * V, g);
        load16<T>(gu + (int64_t)b * x_rs + K + v * V, u);
#pragma unroll
        for (int e = 0; e < V; ++e) g[e] = Elem<T>::round(g[e] / (1.0f + expf(-g[e]))) * u[e];
        store16<T>(xs + b * K + v * V, g);
      }
  } else {
    const S* x = reinterpret_cast<const S*>(x_);
#pragma unroll
    for (int b = 0; b < B; ++b)
      for (int v = tid; v < nvec; v += kGemvThreads)
        *reinterpret_cast<uint4*>(xs + b * K + v * V) = *reinterpret_cast<const uint4*>(x + (int64_t)b * x_rs + v * V);
  }
}

// the SiLU-pair epilogue of a fused gate|up weight: cast(cast(silu(cast(y_gate))) * cast(y_up)) before the final cast of the store (DML:328)
template <typename T>
__device__ __forceinline__ float gemv_silu_pair(float acc_gate, float acc_up) {
  const float g = Elem<T>::round(acc_gate), u = Elem<T>::round(acc_up);
  return Elem<T>::round(g / (1.0f + expf(-g))) * u;
}

}  // namespace dl
