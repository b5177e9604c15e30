// Split-K reduce shared by the small-M GEMMs (dl_gemm_smallm, dl_gemm_mx8): the fp32 partial sums [slices][M][N] of a launch are added in slice order
// (deterministic) and rounded once to the output dtype.
#pragma once
#include "dl_common.h"

namespace dl {

// Y[m,n] = cast(sum_s part[s,m,n]) in slice order.  N % 4 == 0.
template <typename T>
__global__ __launch_bounds__(256) void gemm_smallm_reduce_kernel(const float* __restrict__ part, int n_slices, int M, int N,
                                                                  void* __restrict__ Y_, int64_t ldy) {
  const int64_t nq = (int64_t)M * (N / 4);
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < nq; idx += (int64_t)gridDim.x * 256) {
    const int64_t m = idx / (N / 4);
    const int n = (int)(idx - m * (N / 4)) * 4;
    float4 s = *reinterpret_cast<const float4*>(part + m * N + n);
    for (int k0 = 1; k0 < n_slices; k0 += 8) {  // the loads of up to eight slices are in flight together; the additions stay in slice order
      float4 v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const float4*>(part + ((int64_t)(k0 + j < n_slices ? k0 + j : k0) * M + m) * N + n);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (k0 + j < n_slices) {
          s.x += v[j].x;
          s.y += v[j].y;
          s.z += v[j].z;
          s.w += v[j].w;
        }
    }
    store1<T>(Y_, m * ldy + n, s.x);
    store1<T>(Y_, m * ldy + n + 1, s.y);
    store1<T>(Y_, m * ldy + n + 2, s.z);
    store1<T>(Y_, m * ldy + n + 3, s.w);
  }
}

template <typename T>
static void sm_reduce(float* part, void* Y, int64_t ldy, int M, int N, int n_slices, hipStream_t st) {
  if (n_slices > 1) {
    const int64_t nq = (int64_t)M * (N / 4);
    const int64_t blocks = (nq + 255) / 256;
    hipLaunchKernelGGL((gemm_smallm_reduce_kernel<T>), dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, st, part, n_slices, M, N, Y,
                       ldy);
  }
}

}  // namespace dl
