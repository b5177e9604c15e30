// dl_kv_place: length-aware, row-mapped copy of a KV slab -- how a prefill made on a source cache reaches its rows of a wider decode cache (the pairs of a guided
// generate(): the prompts' rows and the negative prompts' rows), and how the conditional rows leave it again as the caller's cache.  Byte-addressed like
// dl_kv_fork, so one entry serves every storage (16-bit / fp32 slabs, MXFP8 codes, their scale bytes).
//
// One workgroup owns one chunk of the live byte span of one (layer, plane, map entry, head): source row src_rows[i] goes to destination row dst_rows[i].  The
// span length and the row maps come from device memory, so the launch is capturable: the grid is sized from the host bound max_len and workgroups past a row's
// span leave.  A map entry outside either cache is skipped, never dereferenced.  No workspace, no atomics, every loop has a workgroup-uniform trip count.
#include "dl_common.h"

namespace dl {
namespace {

constexpr int kPlaceThreads = 256;
constexpr int kPlaceIters = 4;  // accesses per thread and chunk: all loads of a chunk are in flight before its first store

template <int W>
struct PlaceWord;
template <>
struct PlaceWord<16> {
  using type = uint4;
};
template <>
struct PlaceWord<8> {
  using type = uint2;
};
template <>
struct PlaceWord<4> {
  using type = uint32_t;
};
template <>
struct PlaceWord<2> {
  using type = uint16_t;
};
template <>
struct PlaceWord<1> {
  using type = uint8_t;
};

struct PlaceArgs {
  const uint8_t* src;
  uint8_t* dst;
  int64_t ss_l, ss_p, ss_b, ss_h;  // bytes
  int64_t ds_l, ds_p, ds_b, ds_h;
  int sparse_layer, B_src, B_dst, n_kv_heads;
  int row_bytes, cap;  // cap = min(src_T_cap, dst_T_cap, max_len): slots
  const int32_t *src_rows, *dst_rows;
  const int32_t* src_lens;
  int64_t src_lens_stride;
  int32_t* dst_lens;
  int64_t dst_lens_stride;
};

// grid: x = chunks of the longest possible span, y = map entry * n_kv_heads + head, z = layer * 2 + plane.  W: bytes per access; both bases and all eight
// strides are multiples of W (the host picks the widest such W).
template <int W>
__global__ __launch_bounds__(kPlaceThreads) void kv_place_kernel(PlaceArgs a) {
  using word = typename PlaceWord<W>::type;
  constexpr int64_t kChunk = (int64_t)kPlaceThreads * kPlaceIters * W;
  const int tid = threadIdx.x;
  const int i = blockIdx.y / a.n_kv_heads, h = blockIdx.y % a.n_kv_heads;
  const int l = blockIdx.z >> 1, p = blockIdx.z & 1;
  const int sb = a.src_rows[i], db = a.dst_rows[i];
  if (sb < 0 || sb >= a.B_src || db < 0 || db >= a.B_dst) return;  // (workgroup-uniform) an entry outside its cache is skipped
  if (a.dst_lens != nullptr && blockIdx.x == 0 && blockIdx.z == 0 && h == 0 && tid < 2) {  // one writer per (group, entry)
    a.dst_lens[tid * a.dst_lens_stride + db] = a.src_lens[tid * a.src_lens_stride + sb];
  }
  const int g = l >= a.sparse_layer ? 1 : 0;
  int len = a.src_lens[g * a.src_lens_stride + sb];
  len = len < 0 ? 0 : (len > a.cap ? a.cap : len);
  const int64_t span = (int64_t)len * a.row_bytes;
  const int64_t start = (int64_t)blockIdx.x * kChunk;
  if (start >= span) return;  // (workgroup-uniform)
  const uint8_t* s = a.src + l * a.ss_l + p * a.ss_p + sb * a.ss_b + h * a.ss_h;
  uint8_t* d = a.dst + l * a.ds_l + p * a.ds_p + db * a.ds_b + h * a.ds_h;
  word v[kPlaceIters];
  bool in[kPlaceIters];
#pragma unroll
  for (int k = 0; k < kPlaceIters; ++k) {
    const int64_t off = start + ((int64_t)k * kPlaceThreads + tid) * W;
    in[k] = off + W <= span;
    v[k] = in[k] ? *reinterpret_cast<const word*>(s + off) : word{};
  }
#pragma unroll
  for (int k = 0; k < kPlaceIters; ++k) {
    const int64_t off = start + ((int64_t)k * kPlaceThreads + tid) * W;
    if (in[k]) *reinterpret_cast<word*>(d + off) = v[k];
  }
  if constexpr (W > 1) {
    // the span's last (span % W) bytes, byte by byte, by the workgroup whose chunk they start in
    const int64_t whole = span - span % W;
    if (whole >= start && whole < start + kChunk && whole + tid < span) d[whole + tid] = s[whole + tid];
  }
}

}  // namespace
}  // namespace dl

extern "C" int dl_kv_place(const void* src, void* dst, int64_t src_stride_l, int64_t src_stride_p, int64_t src_stride_b, int64_t src_stride_h,
                           int64_t dst_stride_l, int64_t dst_stride_p, int64_t dst_stride_b, int64_t dst_stride_h, int n_layers, int sparse_layer, int B_src,
                           int B_dst, int n_map, const int32_t* src_rows, const int32_t* dst_rows, int n_kv_heads, int row_bytes, int src_T_cap, int dst_T_cap,
                           const int32_t* src_lens, int64_t src_lens_stride, int32_t* dst_lens, int64_t dst_lens_stride, int max_len, void* stream) {
  using namespace dl;
  DL_REQUIRE(src && dst && src_lens && src_rows && dst_rows, "dl_kv_place: NULL pointer");
  DL_REQUIRE(n_map >= 1 && B_src >= 1 && B_dst >= 1 && row_bytes >= 1 && n_kv_heads >= 1 && n_layers >= 1,
             "dl_kv_place: bad shape (n_map=%d B_src=%d B_dst=%d row_bytes=%d n_kv_heads=%d n_layers=%d)", n_map, B_src, B_dst, row_bytes, n_kv_heads, n_layers);
  DL_REQUIRE(sparse_layer >= 0 && sparse_layer <= n_layers, "dl_kv_place: sparse_layer=%d outside [0, %d]", sparse_layer, n_layers);
  DL_REQUIRE(src_stride_l >= 0 && src_stride_p >= 0 && src_stride_b >= 0 && src_stride_h >= 0 && dst_stride_l >= 0 && dst_stride_p >= 0 && dst_stride_b >= 0 &&
                 dst_stride_h >= 0 && src_lens_stride >= 0 && dst_lens_stride >= 0,
             "dl_kv_place: negative stride");
  DL_REQUIRE(src_T_cap >= 0 && dst_T_cap >= 0 && max_len >= 0, "dl_kv_place: negative capacity");
  DL_REQUIRE((int64_t)n_map * n_kv_heads <= 65535 && n_layers <= 32767, "dl_kv_place: %d entries x %d heads / %d layers exceed the grid", n_map, n_kv_heads, n_layers);
  PlaceArgs a{(const uint8_t*)src, (uint8_t*)dst, src_stride_l, src_stride_p, src_stride_b, src_stride_h, dst_stride_l, dst_stride_p, dst_stride_b, dst_stride_h,
              sparse_layer, B_src, B_dst, n_kv_heads, row_bytes, 0, src_rows, dst_rows, src_lens, src_lens_stride, dst_lens, dst_lens_stride};
  a.cap = src_T_cap < dst_T_cap ? src_T_cap : dst_T_cap;
  a.cap = a.cap < max_len ? a.cap : max_len;
  const uint64_t bits = (uint64_t)(uintptr_t)src | (uint64_t)(uintptr_t)dst | (uint64_t)src_stride_l | (uint64_t)src_stride_p | (uint64_t)src_stride_b | (uint64_t)src_stride_h |
                        (uint64_t)dst_stride_l | (uint64_t)dst_stride_p | (uint64_t)dst_stride_b | (uint64_t)dst_stride_h;
  const int W = (bits & 15) == 0 ? 16 : (bits & 7) == 0 ? 8 : (bits & 3) == 0 ? 4 : (bits & 1) == 0 ? 2 : 1;
  const int64_t chunk = (int64_t)kPlaceThreads * kPlaceIters * W;
  const int64_t chunks = ((int64_t)a.cap * row_bytes + chunk - 1) / chunk;
  DL_REQUIRE(chunks <= 0x7fffffff, "dl_kv_place: span of %d slots x %d bytes exceeds the grid", a.cap, row_bytes);
  const dim3 grid((unsigned)(chunks < 1 ? 1 : chunks), (unsigned)(n_map * n_kv_heads), (unsigned)(n_layers * 2));  // (>= 1 chunk: the lengths are placed even when nothing is live)
  hipStream_t st = as_stream(stream);
  switch (W) {
    case 16: hipLaunchKernelGGL(kv_place_kernel<16>, grid, dim3(kPlaceThreads), 0, st, a); break;
    case 8: hipLaunchKernelGGL(kv_place_kernel<8>, grid, dim3(kPlaceThreads), 0, st, a); break;
    case 4: hipLaunchKernelGGL(kv_place_kernel<4>, grid, dim3(kPlaceThreads), 0, st, a); break;
    case 2: hipLaunchKernelGGL(kv_place_kernel<2>, grid, dim3(kPlaceThreads), 0, st, a); break;
    default: hipLaunchKernelGGL(kv_place_kernel<1>, grid, dim3(kPlaceThreads), 0, st, a); break;
  }
  DL_CHECK_LAUNCH("dl_kv_place");
  return DL_OK;
}
