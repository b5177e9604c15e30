// Device-side constrained decoding: a deterministic token automaton walked inside the decode graphs (generate(constraint= / guided_choice= /
// allowed_token_ids=)).  One launch per step, behind dl_logits_process (logits_proc.hip) and in front of the step-closing launch (dl_decode_advance in
// advance.hip / dl_decode_sample in sample.hip), which consumes its fp32 output unchanged.  The rule is dynamic_llava_amd/constraints.py (the contract this
// kernel is tested against); in short, per row, with s = the row's step clamped into [0, out_cap]:
//   state = s == 0 ? start[b] : the `next` of the edge of state_hist[b, s - 1] whose token is out_ids[b, s - 1] (DONE when there is none);
//   state_hist[b, s] = state;
//   DONE: y_v = float32(logit_v); else y_v = the state has an edge with token v ? float32(logit_v) : -inf.
//
// The geometry is dl_logits_process's: one workgroup of 256 threads owns kTile consecutive entries of one row, one 16-byte load per thread where the row is
// 16-byte addressable, scalar loads for odd strides, unaligned bases and the row's last partial group.  Every workgroup of a row finds the state itself
// (one binary search in the previous state's sorted edges: uniform over the workgroup) from the slot the PREVIOUS launch wrote, which stream order makes
// visible; only the workgroup of tile 0 stores slot s, so the workgroups of a row never race.  The tile's allowed tokens become a kTile-bit mask in LDS:
// two more binary searches find the state's edges whose tokens fall in [lo, hi), the threads set their bits with LDS atomics, and after a barrier every
// thread stores `bit ? x : -inf` for the entries it loaded -- each element is read and written by the same thread, so `out` may be `logits`.
// The table is device memory the host rewrites between requests and nothing in it is trusted: counts are checked against the caps, every state_ptr value
// against n_edges, every `next` against n_states, and a token is turned into a bit index only after it has been compared with [lo, hi).  A bad table
// behaves as DONE.  No workspace, no global atomics, nothing that synchronises with the host.
#include "dl_common.h"

namespace dl {

constexpr int kLcThreads = 256;
constexpr int kLcPerThread = 8;  // one 16-byte load of a 16-bit row, two of an fp32 row
constexpr int kLcTile = kLcThreads * kLcPerThread;
constexpr int kLcMaskWords = kLcTile / 32;

// first index in [e0, e1) whose token is >= tok (e1 when there is none); the range has been checked against the table
__device__ __forceinline__ int lc_lower_bound(const dl_constraint_table* tab, int e0, int e1, int tok) {
  while (e0 < e1) {
    const int mid = e0 + ((e1 - e0) >> 1);
    if (tab->edges[mid][0] < tok) e0 = mid + 1; else e1 = mid;
  }
  return e0;
}

// state -> its edge range, checked: false (the state counts as DONE) for a state outside [0, ns) or a range outside [0, ne]
__device__ __forceinline__ bool lc_edge_range(const dl_constraint_table* tab, int ns, int ne, int state, int& e0, int& e1) {
  if (state < 0 || state >= ns) return false;
  e0 = tab->state_ptr[state];
  e1 = tab->state_ptr[state + 1];
  return e0 >= 0 && e0 <= e1 && e1 <= ne;
}

template <typename T>
__global__ __launch_bounds__(kLcThreads) void logits_constrain_kernel(const void* logits, int64_t row_stride, int V, float* out, const int64_t* __restrict__ out_ids,
                                                                        int out_cap, const int32_t* __restrict__ step, const dl_constraint_table* __restrict__ tab,
                                                                        const int32_t* __restrict__ start, int32_t* state_hist) {
  constexpr int VE = Elem<T>::kVec;
  using S = typename Elem<T>::storage;
  __shared__ uint32_t mask[kLcMaskWords];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int lo = blockIdx.x * kLcTile;
  const int hi = lo + kLcTile < V ? lo + kLcTile : V;  // this workgroup's range [lo, hi)
  const S* row = reinterpret_cast<const S*>(logits) + (int64_t)b * row_stride;
  float* orow = out + (int64_t)b * V;

  // ---- the row's state: uniform over the workgroup ----
  int s = 0;
  if (step && out_ids) {
    s = step[b];
    s = s < 0 ? 0 : (s > out_cap ? out_cap : s);
  }
  int32_t* hist = state_hist + (int64_t)b * (out_cap + 1);
  const int ns = tab->n_states, ne = tab->n_edges;
  int state = DL_CONSTRAIN_DONE, e0 = 0, e1 = 0;
  if (ns >= 1 && ns <= DL_CONSTRAIN_MAX_STATES && ne >= 0 && ne <= DL_CONSTRAIN_MAX_EDGES) {
    if (s == 0) {
      state = start[b];
    } else {
      const int64_t t = out_ids[(int64_t)b * out_cap + (s - 1)];
      int p0, p1;
      if (t >= 0 && t < V && lc_edge_range(tab, ns, ne, hist[s - 1], p0, p1)) {
        const int i = lc_lower_bound(tab, p0, p1, (int)t);
        if (i < p1 && tab->edges[i][0] == (int)t) state = tab->edges[i][1];
      }
    }
    if (!lc_edge_range(tab, ns, ne, state, e0, e1)) state = DL_CONSTRAIN_DONE;  // (an out-of-range `next`, start or edge range: refused, never followed)
  }
  const bool live = state != DL_CONSTRAIN_DONE;
  if (blockIdx.x == 0 && tid == 0) hist[s] = state;

  // ---- the tile's allowed tokens as a bit mask ----
  if (tid < kLcMaskWords) mask[tid] = 0u;
  __syncthreads();
  if (live) {
    // the two lower bounds (of lo and of hi) in one loop: their loads are independent, so a state with tens of thousands of edges pays one chain of
    // dependent loads, not two
    int i0 = e0, j0 = e1, i1 = e0, j1 = e1;
    while (i0 < j0 || i1 < j1) {
      const int m0 = i0 + ((j0 - i0) >> 1), m1 = i1 + ((j1 - i1) >> 1);
      const int t0 = i0 < j0 ? tab->edges[m0][0] : 0, t1 = i1 < j1 ? tab->edges[m1][0] : 0;  // (m < j <= e1 <= n_edges where it is loaded)
      if (i0 < j0) { if (t0 < lo) i0 = m0 + 1; else j0 = m0; }
      if (i1 < j1) { if (t1 < hi) i1 = m1 + 1; else j1 = m1; }
    }
    for (int i = i0 + tid; i < i1; i += kLcThreads) {
      const int t = tab->edges[i][0];
      if (t >= lo && t < hi) atomicOr(&mask[(t - lo) >> 5], 1u << ((t - lo) & 31));  // (checked again: a table that is not sorted must not index past the mask)
    }
  }
  __syncthreads();

  // ---- convert, mask and store the range ----
  const bool in_vec = (row_stride % VE == 0) && ((reinterpret_cast<uintptr_t>(logits) & 15) == 0);
  const bool out_vec = (V % 4 == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
  const int v0 = lo + tid * kLcPerThread;
  const uint32_t bits = live ? (mask[tid >> 2] >> ((tid & 3) * kLcPerThread)) & 0xffu : 0xffu;  // this thread's eight entries
  if (v0 + kLcPerThread <= V) {
    float f[kLcPerThread];
    if (in_vec) {
#pragma unroll
      for (int c = 0; c < kLcPerThread / VE; ++c) {
        float t[VE];
        load16<T>(row + v0 + c * VE, t);
#pragma unroll
        for (int e = 0; e < VE; ++e) f[c * VE + e] = t[e];
      }
    } else {
#pragma unroll
      for (int e = 0; e < kLcPerThread; ++e) f[e] = Elem<T>::to_f(row[v0 + e]);
    }
#pragma unroll
    for (int e = 0; e < kLcPerThread; ++e) f[e] = ((bits >> e) & 1u) ? f[e] : -INFINITY;
    if (out_vec) {
      *reinterpret_cast<float4*>(orow + v0) = make_float4(f[0], f[1], f[2], f[3]);
      *reinterpret_cast<float4*>(orow + v0 + 4) = make_float4(f[4], f[5], f[6], f[7]);
    } else {
#pragma unroll
      for (int e = 0; e < kLcPerThread; ++e) orow[v0 + e] = f[e];
    }
  } else {
    for (int v = v0; v < V; ++v) {  // the row's last, partial group (v0 >= V: nothing)
      const float x = Elem<T>::to_f(row[v]);
      orow[v] = ((bits >> (v - v0)) & 1u) ? x : -INFINITY;
    }
  }
}

}  // namespace dl

using namespace dl;

static_assert(sizeof(dl_constraint_table) == 4 * (8 + DL_CONSTRAIN_MAX_STATES + 1 + 2 * DL_CONSTRAIN_MAX_EDGES), "dl_constraint_table layout");

extern "C" int dl_logits_constrain(const void* logits, int logits_dtype, int64_t logits_row_stride, int V, int B, float* out, const int64_t* out_ids,
                                   int out_cap, const int32_t* step, const dl_constraint_table* table, const int32_t* start, int32_t* state_hist, void* stream) {
  DL_REQUIRE(logits && out, "dl_logits_constrain: NULL pointer");
  DL_REQUIRE(table && start && state_hist, "dl_logits_constrain: NULL table, start or state_hist");
  DL_REQUIRE(B > 0 && V > 0 && out_cap >= 0, "dl_logits_constrain: bad shape");
  DL_REQUIRE(B <= 65535, "dl_logits_constrain: B=%d exceeds 65535 rows", B);
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)((V + kLcTile - 1) / kLcTile), (unsigned)B);
  DL_DISPATCH_DTYPE(logits_dtype, T, {
    hipLaunchKernelGGL((logits_constrain_kernel<T>), grid, dim3(kLcThreads), 0, st, logits, logits_row_stride, V, out, out_ids, out_cap, step, table, start, state_hist);
  });
  DL_CHECK_LAUNCH("dl_logits_constrain");
  return DL_OK;
}
