// dl_kv_fork: length-aware, replicated copy of a KV slab -- the step between one prefill of B prompts and the decode of B * n_rep sampled answers
// (generate(num_return_sequences=n)).  Byte-addressed, so one entry serves every storage (16-bit / fp32 slabs, MXFP8 codes, their scale bytes).
//
// One workgroup owns one chunk of the live byte span of one (layer, plane, source row, head): it reads the chunk ONCE and stores it n_rep times,
// (1 + n_rep) x live bytes of traffic.  The span length comes from device memory (src_lens), so the launch is capturable: the grid is sized from the
// host bound max_len and workgroups past a row's span leave.  No workspace, no atomics, every loop has a workgroup-uniform trip count.
#include "dl_common.h"

namespace dl {
namespace {

constexpr int kForkThreads = 256;
constexpr int kForkIters = 4;  // accesses per thread and chunk: all loads of a chunk are in flight before its first store

template <int W>
struct ForkWord;
template <>
struct ForkWord<16> {
  using type = uint4;
};
template <>
struct ForkWord<8> {
  using type = uint2;
};
template <>
struct ForkWord<4> {
  using type = uint32_t;
};
template <>
struct ForkWord<2> {
  using type = uint16_t;
};
template <>
struct ForkWord<1> {
  using type = uint8_t;
};

struct ForkArgs {
  const uint8_t* src;
  uint8_t* dst;
  int64_t ss_l, ss_p, ss_b, ss_h;  // bytes
  int64_t ds_l, ds_p, ds_b, ds_h;
  int sparse_layer, B_src, n_rep, n_kv_heads;
  int row_bytes, cap;  // cap = min(src_T_cap, dst_T_cap, max_len): slots
  const int32_t* src_lens;
  int64_t src_lens_stride;
  int32_t* dst_lens;
  int64_t dst_lens_stride;
};

// grid: x = chunks of the longest possible span, y = source row * n_kv_heads + head, z = layer * 2 + plane.  W: bytes per access; both bases and all
// eight strides are multiples of W (the host picks the widest such W), so every plane starts W-aligned and so does every chunk.
template <int W>
__global__ __launch_bounds__(kForkThreads) void kv_fork_kernel(ForkArgs a) {
  using word = typename ForkWord<W>::type;
  constexpr int64_t kChunk = (int64_t)kForkThreads * kForkIters * W;
  const int tid = threadIdx.x;
  const int b = blockIdx.y / a.n_kv_heads, h = blockIdx.y % a.n_kv_heads;
  const int l = blockIdx.z >> 1, p = blockIdx.z & 1;
  if (a.dst_lens != nullptr && blockIdx.x == 0 && blockIdx.z == 0 && h == 0 && tid < 2) {  // one writer per (group, source row): lane g of one workgroup
    const int32_t n = a.src_lens[tid * a.src_lens_stride + b];
    for (int r = 0; r < a.n_rep; ++r) a.dst_lens[tid * a.dst_lens_stride + (int64_t)b * a.n_rep + r] = n;
  }
  const int g = l >= a.sparse_layer ? 1 : 0;
  int len = a.src_lens[g * a.src_lens_stride + b];
  len = len < 0 ? 0 : (len > a.cap ? a.cap : len);
  const int64_t span = (int64_t)len * a.row_bytes;
  const int64_t start = (int64_t)blockIdx.x * kChunk;
  if (start >= span) return;  // (workgroup-uniform)
  const uint8_t* s = a.src + l * a.ss_l + p * a.ss_p + b * a.ss_b + h * a.ss_h;
  uint8_t* d = a.dst + l * a.ds_l + p * a.ds_p + ((int64_t)b * a.n_rep) * a.ds_b + h * a.ds_h;
  word v[kForkIters];
  bool in[kForkIters];
#pragma unroll
  for (int i = 0; i < kForkIters; ++i) {
    const int64_t off = start + ((int64_t)i * kForkThreads + tid) * W;
    in[i] = off + W <= span;
    v[i] = in[i] ? *reinterpret_cast<const word*>(s + off) : word{};
  }
  for (int r = 0; r < a.n_rep; ++r) {
    uint8_t* dr = d + r * a.ds_b;
#pragma unroll
    for (int i = 0; i < kForkIters; ++i) {
      const int64_t off = start + ((int64_t)i * kForkThreads + tid) * W;
      if (in[i]) *reinterpret_cast<word*>(dr + off) = v[i];
    }
  }
  if constexpr (W > 1) {
    // the span's last (span % W) bytes, byte by byte, by the workgroup whose chunk they start in
    const int64_t whole = span - span % W;
    if (whole >= start && whole < start + kChunk && whole + tid < span) {
      const uint8_t t = s[whole + tid];
      for (int r = 0; r < a.n_rep; ++r) d[r * a.ds_b + whole + tid] = t;
    }
  }
}

}  // namespace
}  // namespace dl

extern "C" int dl_kv_fork(const void* src, void* dst, int64_t src_stride_l, int64_t src_stride_p, int64_t src_stride_b, int64_t src_stride_h,
                          int64_t dst_stride_l, int64_t dst_stride_p, int64_t dst_stride_b, int64_t dst_stride_h, int n_layers, int sparse_layer, int B_src,
                          int n_rep, int n_kv_heads, int row_bytes, int src_T_cap, int dst_T_cap, const int32_t* src_lens, int64_t src_lens_stride,
                          int32_t* dst_lens, int64_t dst_lens_stride, int max_len, void* stream) {
  using namespace dl;
  DL_REQUIRE(src && dst && src_lens, "dl_kv_fork: NULL pointer");
  DL_REQUIRE(n_rep >= 1 && B_src >= 1 && row_bytes >= 1 && n_kv_heads >= 1 && n_layers >= 1, "dl_kv_fork: bad shape (n_rep=%d B_src=%d row_bytes=%d n_kv_heads=%d n_layers=%d)",
             n_rep, B_src, row_bytes, n_kv_heads, n_layers);
  DL_REQUIRE(sparse_layer >= 0 && sparse_layer <= n_layers, "dl_kv_fork: sparse_layer=%d outside [0, %d]", sparse_layer, n_layers);
  DL_REQUIRE(src_stride_l >= 0 && src_stride_p >= 0 && src_stride_b >= 0 && src_stride_h >= 0 && dst_stride_l >= 0 && dst_stride_p >= 0 && dst_stride_b >= 0 &&
                 dst_stride_h >= 0 && src_lens_stride >= 0 && dst_lens_stride >= 0,
             "dl_kv_fork: negative stride");
  DL_REQUIRE(src_T_cap >= 0 && dst_T_cap >= 0 && max_len >= 0, "dl_kv_fork: negative capacity");
  DL_REQUIRE((int64_t)B_src * n_kv_heads <= 65535 && n_layers <= 32767, "dl_kv_fork: %d rows x %d heads / %d layers exceed the grid", B_src, n_kv_heads, n_layers);
  ForkArgs a{(const uint8_t*)src, (uint8_t*)dst, src_stride_l, src_stride_p, src_stride_b, src_stride_h, dst_stride_l, dst_stride_p, dst_stride_b, dst_stride_h,
             sparse_layer, B_src, n_rep, n_kv_heads, row_bytes, 0, src_lens, src_lens_stride, dst_lens, dst_lens_stride};
  a.cap = src_T_cap < dst_T_cap ? src_T_cap : dst_T_cap;
  a.cap = a.cap < max_len ? a.cap : max_len;
  // the widest access both bases and all strides allow (a plane of an imported cache with an odd T_cap, or of 2- / 4-byte scale rows, starts anywhere)
  const uint64_t bits = (uint64_t)(uintptr_t)src | (uint64_t)(uintptr_t)dst | (uint64_t)src_stride_l | (uint64_t)src_stride_p | (uint64_t)src_stride_b | (uint64_t)src_stride_h |
                        (uint64_t)dst_stride_l | (uint64_t)dst_stride_p | (uint64_t)dst_stride_b | (uint64_t)dst_stride_h;
  const int W = (bits & 15) == 0 ? 16 : (bits & 7) == 0 ? 8 : (bits & 3) == 0 ? 4 : (bits & 1) == 0 ? 2 : 1;
  const int64_t chunk = (int64_t)kForkThreads * kForkIters * W;
  const int64_t chunks = ((int64_t)a.cap * row_bytes + chunk - 1) / chunk;
  DL_REQUIRE(chunks <= 0x7fffffff, "dl_kv_fork: span of %d slots x %d bytes exceeds the grid", a.cap, row_bytes);
  const dim3 grid((unsigned)(chunks < 1 ? 1 : chunks), (unsigned)(B_src * n_kv_heads), (unsigned)(n_layers * 2));  // (>= 1 chunk: the lengths are forked even when nothing is live)
  hipStream_t st = as_stream(stream);
  switch (W) {
    case 16: hipLaunchKernelGGL(kv_fork_kernel<16>, grid, dim3(kForkThreads), 0, st, a); break;
    case 8: hipLaunchKernelGGL(kv_fork_kernel<8>, grid, dim3(kForkThreads), 0, st, a); break;
    case 4: hipLaunchKernelGGL(kv_fork_kernel<4>, grid, dim3(kForkThreads), 0, st, a); break;
    case 2: hipLaunchKernelGGL(kv_fork_kernel<2>, grid, dim3(kForkThreads), 0, st, a); break;
    default: hipLaunchKernelGGL(kv_fork_kernel<1>, grid, dim3(kForkThreads), 0, st, a); break;
  }
  DL_CHECK_LAUNCH("dl_kv_fork");
  return DL_OK;
}
