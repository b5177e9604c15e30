// Batch-1 decode weight streaming on LOSSLESS 12-bit packed bf16 rows (the format: dynamic_llava_amd/bf16pack.py).  A bf16 weight keeps its low byte
// and 4 bits of its high byte (sign + a 3-bit offset into the matrix's window of 16 exponents); a lane rebuilds the exact 16-byte bf16 chunk in
// registers (two byte-parallel adds / masks and four v_perm_b32 per chunk) and then runs the SAME arithmetic as gemv.hip: same chunk -> lane map,
// same rising chunk order from acc = 0, same four v_dot2c_f32_bf16 per chunk, same wave_sum, same prologues (gemv_prologue.h) and epilogues.  The
// result is bit-identical to dl_gemv on the unpacked weights while the launch streams 0.75 of the bytes (+ the raw copies of the ~4 % of spans
// that hold an escape).
//
// Escapes: a span (64 chunks, v = lane + 64 c) with an element outside the window is read raw from the matrix's pool.  The row header {span mask,
// first pool span} of the wave's NEXT rows is requested together with this pass's weights, so that the raw 16 bytes per lane of a flagged span
// (the first flagged span of each row of the pass; more than one is rare and pays a dependent load) travel with the packed bytes.  The branch is
// wave-uniform.  Pool indices are clamped to the pool on the device: a corrupt header can give wrong numbers, never an out-of-bounds address.
//
// No lane ever forms an address outside the row it reads: pairs of full spans are read by all 64 lanes (16 + 8 bytes each), what is left of a
// segment is read per chunk (8 + 4 bytes) under `chunk < row end`; row indices -- of the prefetched headers too -- are clamped to N - 1.
#include "gemv_dot.h"
#include "gemv_prologue.h"
#include "../../include/dynllava.h"

namespace dl {

constexpr int kPkPairBytes = 1536;  // two spans: 64 x 16 low bytes + 64 x 8 nibble bytes
constexpr int kPkSpanBytes = 1024;  // a raw span in the pool

struct PkMat {
  const unsigned char* data;  // [N][K * 3 / 2]
  const uint2* hdr;           // [N] {span mask, first pool span}
  const unsigned char* pool;  // [pool_last + 1][1024]
  int64_t row_bytes;
  uint32_t pool_last;
  uint32_t hb4;  // hb in every byte
};

__device__ __forceinline__ uint2 ldg_nt8(const void* p) {
  typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
  const u32x2_t r = __builtin_nontemporal_load(reinterpret_cast<const u32x2_t*>(p));
  return make_uint2(r.x, r.y);
}
__device__ __forceinline__ uint32_t ldg_nt4(const void* p) { return __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p)); }

// the low bytes of 8 elements (lo0: 0..3, lo1: 4..7) and their 4 pre-spread nibble bytes -> the 16-byte bf16 chunk
__device__ __forceinline__ uint4 pk_decode(uint32_t lo0, uint32_t lo1, uint32_t nb, uint32_t hb4) {
  const uint32_t h0 = ((nb & 0x07070707u) + hb4) | ((nb & 0x08080808u) << 4);
  const uint32_t h1 = (((nb >> 4) & 0x07070707u) + hb4) | (nb & 0x80808080u);
  // v_perm_b32: selector bytes 0..3 take the second operand's bytes, 4..7 the first's
  return make_uint4(__builtin_amdgcn_perm(h0, lo0, 0x05010400u), __builtin_amdgcn_perm(h0, lo0, 0x07030602u),
                    __builtin_amdgcn_perm(h1, lo1, 0x05010400u), __builtin_amdgcn_perm(h1, lo1, 0x07030602u));
}

// A row's header as wave-uniform scalars
struct PkHdr {
  uint32_t mask, off;
};
__device__ __forceinline__ PkHdr pk_uniform(const uint2 h) {
  PkHdr r;
  r.mask = __builtin_amdgcn_readfirstlane(h.x);
  r.off = __builtin_amdgcn_readfirstlane(h.y);
  return r;
}
// the lane's 16 bytes of span s of a row whose header is h (s is flagged in h.mask)
__device__ __forceinline__ const unsigned char* pk_raw_addr(const PkMat& m, const PkHdr& h, int s, int lane) {
  uint32_t idx = h.off + (uint32_t)__builtin_popcount(h.mask & ((1u << s) - 1u));
  idx = idx < m.pool_last ? idx : m.pool_last;
  return m.pool + (int64_t)idx * kPkSpanBytes + lane * 16;
}

// A *slot* is a pair of spans of one row in flight: chunks c = 2 slot (lo.x, lo.y, nb.x) and 2 slot + 1 (lo.z, lo.w, nb.y).  A *pass* holds SLOTS slots of
// each of R rows, requested slot-major (the order they are consumed in), the rows' flagged spans of the pass and the raw chunk of each row's first.
template <int R, int SLOTS>
struct PkPass {
  uint4 lo[SLOTS][R];
  uint2 nb[SLOTS][R];
  uint4 raw0[R];
  uint32_t fm[R];
};

// Requests the lane's bytes of pair `p` of a segment (`seg`: its first byte, nc chunks).  TAIL: the segment may end in fewer than 128 chunks, which are
// read per chunk (lanes past the end read nothing and hold zeros: they decode to a finite positive number, and their x is zero).
template <bool TAIL>
__device__ __forceinline__ void pk_request_slot(uint4& lo, uint2& nb, const unsigned char* seg, int nc, int p, int lane) {
  const int P = nc >> 7;
  if (!TAIL || p < P) {  // (TAIL = false: the caller knows that pair p exists)
    lo = ldg_nt(seg + (int64_t)p * kPkPairBytes + lane * 16);
    nb = ldg_nt8(seg + (int64_t)p * kPkPairBytes + 1024 + lane * 8);
  } else {  // at most ONE slot of a segment is not a whole pair: the nt < 128 chunks behind the pairs, read by lanes t < nt (and t + 64 < nt)
    const int nt = nc - 128 * P;
    const unsigned char* tail = seg + (int64_t)P * kPkPairBytes;
    uint2 l0 = make_uint2(0u, 0u), l1 = make_uint2(0u, 0u);
    uint32_t n0 = 0u, n1 = 0u;
    if (p == P && lane < nt) {
      l0 = ldg_nt8(tail + lane * 8);
      n0 = ldg_nt4(tail + nt * 8 + lane * 4);
    }
    if (p == P && lane + 64 < nt) {
      l1 = ldg_nt8(tail + (lane + 64) * 8);
      n1 = ldg_nt4(tail + nt * 8 + (lane + 64) * 4);
    }
    lo = make_uint4(l0.x, l0.y, l1.x, l1.y);
    nb = make_uint2(n0, n1);
  }
}

// The flagged spans of each row among the pass's 2 SLOTS spans from span s0 on (bit c: chunk slot c; nsp: spans of the segment left from s0 on -- a later
// span belongs to another wave), and the request for the raw chunk of the first one.
template <int R, int SLOTS>
__device__ __forceinline__ void pk_request_raw(PkPass<R, SLOTS>& ps, const PkMat& m, const PkHdr (&h)[R], int s0, int nsp, int lane) {
  const uint32_t keep = nsp >= 2 * SLOTS ? ((1u << (2 * SLOTS)) - 1u) : ((1u << nsp) - 1u);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    ps.fm[r] = (h[r].mask >> s0) & keep;
    ps.raw0[r] = make_uint4(0u, 0u, 0u, 0u);
    if (ps.fm[r] != 0u) ps.raw0[r] = ldg_nt(pk_raw_addr(m, h[r], s0 + __builtin_ctz(ps.fm[r]), lane));
  }
}

// acc[r] += the pass's chunks of row r . x, in rising chunk order; slots [0, nvalid).  x(c): the x chunk of chunk slot c.  The usual pass (no flagged
// span in any row) is straight-line code, held slot by slot to the order decode -> dot so that the decoded words of later slots do not pile up in registers.
template <int R, int SLOTS, typename XF>
__device__ __forceinline__ void pk_pass_dot(const PkMat& m, const PkPass<R, SLOTS>& ps, const PkHdr (&h)[R], int s0, int nvalid, int lane, float (&acc)[R], XF x) {
  uint32_t any = 0u;
#pragma unroll
  for (int r = 0; r < R; ++r) any |= ps.fm[r];
  if (any == 0u) {
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
      if (i < nvalid) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const uint4 xv = x(2 * i + j);
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const uint4& lo = ps.lo[i][r];
            const uint2& nb = ps.nb[i][r];
            const uint4 w = j ? pk_decode(lo.z, lo.w, nb.y, m.hb4) : pk_decode(lo.x, lo.y, nb.x, m.hb4);
            acc[r] = dot16<bf16_t>(w, xv, acc[r]);
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  } else {
    int first[R];
#pragma unroll
    for (int r = 0; r < R; ++r) first[r] = ps.fm[r] ? __builtin_ctz(ps.fm[r]) : -1;
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
      if (i < nvalid) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int c = 2 * i + j;
          const uint4 xv = x(c);
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const uint4& lo = ps.lo[i][r];
            const uint2& nb = ps.nb[i][r];
            uint4 w = j ? pk_decode(lo.z, lo.w, nb.y, m.hb4) : pk_decode(lo.x, lo.y, nb.x, m.hb4);
            if ((ps.fm[r] >> c) & 1u) w = c == first[r] ? ps.raw0[r] : ldg_nt(pk_raw_addr(m, h[r], s0 + c, lane));  // (wave-uniform)
            acc[r] = dot16<bf16_t>(w, xv, acc[r]);
          }
        }
      }
    }
  }
}

// ---- plain prologue, x in registers (o_proj; K <= 8192): gemv_b1_plain_kernel on packed rows.  RW rows per wave and pass share the x registers,
// which keeps at least as many bytes in flight per lane as the bf16 kernel's one row (RW * XB * 96 against XB * 128) ----
// TF: slots [0, TF) are whole pairs for every K the host sends here (no branch, no tail addresses); later ones may be the tail or empty
template <int XB, int RW, int WPE, int TF>
__global__ __launch_bounds__(kGemvThreads) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void gemv_pk_plain_kernel(PkMat m, int N, int K, const void* __restrict__ x_,
                                                                                                             void* __restrict__ y_) {
  constexpr int SLOTS = XB * 4;
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (a scalar: row addresses stay in SGPRs)
  const int nvec = K / 8;
  const uint16_t* x = reinterpret_cast<const uint16_t*>(x_);
  const int groups = (N + 4 * RW - 1) / (4 * RW);
  auto row_of = [&](int grp, int r) {
    const int n = grp * 4 * RW + wid * RW + r;
    return n < N ? n : N - 1;
  };
  uint2 hraw[RW];
#pragma unroll
  for (int r = 0; r < RW; ++r) hraw[r] = m.hdr[row_of((int)blockIdx.x, r)];
  uint4 xr[XB * 8];
#pragma unroll
  for (int c = 0; c < XB * 8; ++c) {
    const int v = lane + 64 * c;
    xr[c] = v < nvec ? *reinterpret_cast<const uint4*>(x + (int64_t)v * 8) : make_uint4(0u, 0u, 0u, 0u);
  }
  for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {
    PkPass<RW, SLOTS> ps;
    PkHdr h[RW];
#pragma unroll
    for (int i = 0; i < SLOTS; ++i)
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        const unsigned char* seg = m.data + (int64_t)row_of(grp, r) * m.row_bytes;
        if (i < TF) pk_request_slot<false>(ps.lo[i][r], ps.nb[i][r], seg, nvec, i, lane);
        else pk_request_slot<true>(ps.lo[i][r], ps.nb[i][r], seg, nvec, i, lane);
      }
#pragma unroll
    for (int r = 0; r < RW; ++r) h[r] = pk_uniform(hraw[r]);
    pk_request_raw<RW, SLOTS>(ps, m, h, 0, (nvec + 63) >> 6, lane);
    const int nxt = grp + (int)gridDim.x < groups ? grp + (int)gridDim.x : grp;
#pragma unroll
    for (int r = 0; r < RW; ++r) hraw[r] = m.hdr[row_of(nxt, r)];
    float acc[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) acc[r] = 0.f;
    pk_pass_dot<RW, SLOTS>(m, ps, h, 0, SLOTS, lane, acc, [&](int c) -> const uint4& { return xr[c]; });
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      acc[r] = wave_sum(acc[r]);
      const int n = grp * 4 * RW + wid * RW + r;
      if (lane == 0 && n < N) store1<bf16_t>(y_, n, acc[r]);
    }
  }
}

// ---- plain prologue, long rows (down_proj; 8192 < K <= 16384): gemv_b1_plain_halves_kernel on packed rows.  A row is shared by the two waves of a
// pair -- the row's two segments -- and the even wave adds the partial sums low half first.  RW rows per pair and pass. ----
template <int C, int RW, int WPE, int TF>
__global__ __launch_bounds__(kGemvThreads) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void gemv_pk_halves_kernel(PkMat m, int N, int K, const void* __restrict__ x_,
                                                                                                              void* __restrict__ y_) {
  static_assert(C % 2 == 0, "whole slots");
  constexpr int SLOTS = C / 2;
  __shared__ float part[RW][kGemvThreads / 64];
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (a scalar: row addresses stay in SGPRs)
  const int half = wid & 1, pr = wid >> 1;
  const int nvec = K / 8;
  const int hv = ((nvec + 1) / 2 + 63) / 64 * 64;  // chunks of the low half (whole lane sets)
  const int v0 = half * hv, v1 = half ? nvec : (hv < nvec ? hv : nvec);
  const uint16_t* x = reinterpret_cast<const uint16_t*>(x_);
  constexpr int RPW = RW * kGemvThreads / 128;  // rows per workgroup pass
  const int groups = (N + RPW - 1) / RPW;
  auto row_of = [&](int grp, int r) {
    const int n = grp * RPW + pr * RW + r;
    return n < N ? n : N - 1;
  };
  uint2 hraw[RW];
#pragma unroll
  for (int r = 0; r < RW; ++r) hraw[r] = m.hdr[row_of((int)blockIdx.x, r)];
  uint4 xr[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int v = v0 + lane + 64 * c;
    xr[c] = v < v1 ? *reinterpret_cast<const uint4*>(x + (int64_t)v * 8) : make_uint4(0u, 0u, 0u, 0u);
  }
  for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {
    PkPass<RW, SLOTS> ps;
    PkHdr h[RW];
#pragma unroll
    for (int i = 0; i < SLOTS; ++i)
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        const unsigned char* seg = m.data + (int64_t)row_of(grp, r) * m.row_bytes + (int64_t)v0 * 12;
        if (i < TF) pk_request_slot<false>(ps.lo[i][r], ps.nb[i][r], seg, v1 - v0, i, lane);
        else pk_request_slot<true>(ps.lo[i][r], ps.nb[i][r], seg, v1 - v0, i, lane);
      }
#pragma unroll
    for (int r = 0; r < RW; ++r) h[r] = pk_uniform(hraw[r]);
    pk_request_raw<RW, SLOTS>(ps, m, h, v0 >> 6, (v1 - v0 + 63) >> 6, lane);
    const int nxt = grp + (int)gridDim.x < groups ? grp + (int)gridDim.x : grp;
#pragma unroll
    for (int r = 0; r < RW; ++r) hraw[r] = m.hdr[row_of(nxt, r)];
    float acc[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) acc[r] = 0.f;
    pk_pass_dot<RW, SLOTS>(m, ps, h, v0 >> 6, SLOTS, lane, acc, [&](int c) -> const uint4& { return xr[c]; });
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      acc[r] = wave_sum(acc[r]);
      if (lane == 0 && half) part[r][wid] = acc[r];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      const int n = grp * RPW + pr * RW + r;
      if (lane == 0 && !half && n < N) store1<bf16_t>(y_, n, acc[r] + part[r][wid + 1]);
    }
    __syncthreads();
  }
}

// ---- add + rmsnorm prologue, x in LDS (gate|up with the SiLU-pair epilogue, the vocabulary projection, the unfused q|k|v): gemv_body<T, 1, 1, PAIR, 2, 4>
// on packed rows, K % 1024 == 0 (whole pairs).  Two rows per wave, up to SLOTS = 4 pairs (8 spans) of each in flight: 192 bytes per lane against the bf16
// body's 2 x 4 x 16.  Half of the first pass is requested before the prologue (the whole of it would not fit beside the prologue's registers). ----
template <bool PAIR>
__global__ __launch_bounds__(kGemvThreads) __attribute__((amdgpu_waves_per_eu(4, 4))) void gemv_pk_addnorm_kernel(PkMat m, int N, int K, const void* __restrict__ h_,
                                                                                                            void* __restrict__ h_out_, const void* __restrict__ delta_,
                                                                                                            const void* __restrict__ nw_, float eps, void* __restrict__ y_) {
  constexpr int R = 2, SLOTS = 4, PRE = 2;
  using S = Elem<bf16_t>::storage;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  S* xs = reinterpret_cast<S*>(smem);  // [K]
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // (a scalar: row addresses stay in SGPRs)
  const int bid = blockIdx.x, nblk = gridDim.x;
  const int nvec = K / 8, P = nvec >> 7;
  const int n_out = PAIR ? N / 2 : N;
  constexpr int RW = PAIR ? 1 : R;
  const int groups = (n_out + 4 * RW - 1) / (4 * RW);
  auto row_of = [&](int grp, int r) {  // gemv_body's row choice
    const int n0 = grp * 4 * RW + wid * RW;
    int n = PAIR ? (n0 + r * n_out) : (n0 + r);
    n = n < N ? n : N - 1;
    if (PAIR && n0 >= n_out) n = r * n_out;
    return n;
  };
  // the weight stream starts BEFORE the prologue (as in gemv_body): the first pairs and the headers of this workgroup's first rows
  PkPass<R, SLOTS> ps;
  uint2 hraw[R];
  const bool have_pre = bid < groups;
  if (have_pre) {
#pragma unroll
    for (int r = 0; r < R; ++r) hraw[r] = m.hdr[row_of(bid, r)];
#pragma unroll
    for (int i = 0; i < PRE; ++i)
      if (i < P) {
#pragma unroll
        for (int r = 0; r < R; ++r) pk_request_slot<false>(ps.lo[i][r], ps.nb[i][r], m.data + (int64_t)row_of(bid, r) * m.row_bytes, nvec, i, lane);
      }
  }
  gemv_build_x<bf16_t, 1, 1>(xs, red, K, nullptr, 0, h_, h_out_, delta_, nw_, eps, bid);
  __syncthreads();

  bool first = have_pre;
  for (int grp = bid; grp < groups; grp += nblk) {
    const int n0 = grp * 4 * RW + wid * RW;
    const unsigned char* wp[R];
    PkHdr h[R];
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      wp[r] = m.data + (int64_t)row_of(grp, r) * m.row_bytes;
      h[r] = pk_uniform(hraw[r]);
      acc[r] = 0.f;
    }
    const int nxt = grp + nblk < groups ? grp + nblk : grp;
    for (int p0 = 0; p0 < P; p0 += SLOTS) {
      const int i0 = first ? PRE : 0;  // the first slots of the workgroup's first pass are in flight since before the prologue
      first = false;
#pragma unroll
      for (int i = 0; i < SLOTS; ++i)
        if (i >= i0 && p0 + i < P) {
#pragma unroll
          for (int r = 0; r < R; ++r) pk_request_slot<false>(ps.lo[i][r], ps.nb[i][r], wp[r], nvec, p0 + i, lane);
        }
      pk_request_raw<R, SLOTS>(ps, m, h, 2 * p0, 2 * (P - p0), lane);
      if (p0 == 0) {  // the next rows' headers travel with this pass's weights
#pragma unroll
        for (int r = 0; r < R; ++r) hraw[r] = m.hdr[row_of(nxt, r)];
      }
      pk_pass_dot<R, SLOTS>(m, ps, h, 2 * p0, P - p0, lane, acc,
                            [&](int c) { return *reinterpret_cast<const uint4*>(xs + (int64_t)(lane + 64 * (2 * p0 + c)) * 8); });
    }
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = wave_sum(acc[r]);
    if (lane == 0) {
      if constexpr (PAIR) {
        if (n0 < n_out) store1<bf16_t>(y_, n0, gemv_silu_pair<bf16_t>(acc[0], acc[1]));
      } else {
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (n0 + r < N) store1<bf16_t>(y_, n0 + r, acc[r]);
      }
    }
  }
}

constexpr int kPkGridCap = 1024;  // dl_gemv's default: 4 workgroups per CU

}  // namespace dl

using namespace dl;

extern "C" int dl_gemv_pk(int mode, const void* data, int64_t data_bytes, const void* hdr, int64_t hdr_rows, const void* pool, int64_t pool_spans, int hb, int N,
                          int K, const void* x, const void* h_in, void* h_out, const void* delta, const void* norm_w, float eps, void* y, int B, int dtype,
                          int grid_cap, void* stream) {
  DL_REQUIRE(data && hdr && pool && y, "dl_gemv_pk: NULL pointer");
  DL_REQUIRE(dtype == DL_BF16, "dl_gemv_pk: bf16 only (dtype %d)", dtype);
  DL_REQUIRE(B == 1, "dl_gemv_pk: batch 1 only (B=%d)", B);
  DL_REQUIRE(N > 0 && K > 0 && K % 64 == 0 && K <= 16384 && grid_cap >= 0, "dl_gemv_pk: bad shape N=%d K=%d", N, K);
  DL_REQUIRE(hb >= 0 && hb <= 120, "dl_gemv_pk: hb=%d is outside [0, 120]", hb);
  const int64_t row_bytes = (int64_t)K * 3 / 2;
  DL_REQUIRE(data_bytes >= (int64_t)N * row_bytes, "dl_gemv_pk: %lld packed bytes, %d rows of K=%d need %lld", (long long)data_bytes, N, K, (long long)((int64_t)N * row_bytes));
  DL_REQUIRE(hdr_rows >= N, "dl_gemv_pk: %lld row headers for %d rows", (long long)hdr_rows, N);
  DL_REQUIRE(pool_spans >= 1 && pool_spans < ((int64_t)1 << 31), "dl_gemv_pk: the pool must hold at least one span (%lld)", (long long)pool_spans);
  DL_REQUIRE(((uintptr_t)data | (uintptr_t)pool) % 16 == 0 && (uintptr_t)hdr % 8 == 0, "dl_gemv_pk: data / pool must be 16-byte aligned, hdr 8-byte");
  const int pro = mode & 3;
  const bool pair = (mode & DL_GEMV_OUT_SILU_PAIR) != 0;
  DL_REQUIRE((mode & ~(3 | DL_GEMV_OUT_SILU_PAIR)) == 0 && (pro == DL_GEMV_PLAIN || pro == DL_GEMV_ADDNORM), "dl_gemv_pk: bad mode %d", mode);
  DL_REQUIRE(!pair || (pro == DL_GEMV_ADDNORM && N % 2 == 0), "dl_gemv_pk: SILU_PAIR needs the ADDNORM prologue and an even N");
  if (grid_cap == 0) grid_cap = kPkGridCap;
  PkMat m;
  m.data = reinterpret_cast<const unsigned char*>(data);
  m.hdr = reinterpret_cast<const uint2*>(hdr);
  m.pool = reinterpret_cast<const unsigned char*>(pool);
  m.row_bytes = row_bytes;
  m.pool_last = (uint32_t)(pool_spans - 1);
  m.hb4 = (uint32_t)hb * 0x01010101u;
  hipStream_t st = as_stream(stream);
  if (pro == DL_GEMV_ADDNORM) {
    DL_REQUIRE(h_in && norm_w, "dl_gemv_pk: missing operand for mode %d", mode);
    DL_REQUIRE(!delta || (h_out && h_out != h_in), "dl_gemv_pk: h_out must be a distinct buffer when delta is given");
    DL_REQUIRE(K % 1024 == 0 && K <= 8192, "dl_gemv_pk: the ADDNORM prologue takes K %% 1024 == 0, K <= 8192 (K=%d)", K);
    const int n_out = pair ? N / 2 : N;
    const int per = 4 * (pair ? 1 : 2);
    const int groups = (n_out + per - 1) / per;
    const int grid = groups < grid_cap ? groups : grid_cap;
    const size_t smem = (size_t)K * 2;
    if (pair) hipLaunchKernelGGL((gemv_pk_addnorm_kernel<true>), dim3((unsigned)grid), dim3(kGemvThreads), smem, st, m, N, K, h_in, h_out, delta, norm_w, eps, y);
    else hipLaunchKernelGGL((gemv_pk_addnorm_kernel<false>), dim3((unsigned)grid), dim3(kGemvThreads), smem, st, m, N, K, h_in, h_out, delta, norm_w, eps, y);
  } else {
    DL_REQUIRE(x != nullptr, "dl_gemv_pk: missing operand for mode %d", mode);
    DL_REQUIRE((uintptr_t)x % 16 == 0, "dl_gemv_pk: x must be 16-byte aligned");
    // (the plain launches run at most grid_cap / 2 workgroups, as dl_gemv's: two per CU, which leaves them 256 registers)
    const int cap2 = grid_cap / 2 > 0 ? grid_cap / 2 : 1;
    if (K <= 4096) {  // two rows per wave and pass
      const int groups = (N + 7) / 8;
      const dim3 grid((unsigned)(groups < cap2 ? groups : cap2));
      if (K == 4096) hipLaunchKernelGGL((gemv_pk_plain_kernel<1, 2, 2, 4>), grid, dim3(kGemvThreads), 0, st, m, N, K, x, y);
      else hipLaunchKernelGGL((gemv_pk_plain_kernel<1, 2, 2, 0>), grid, dim3(kGemvThreads), 0, st, m, N, K, x, y);
    } else if (K <= 8192) {  // x alone takes 64 registers: one row per wave and pass; K > 4096: at least four whole pairs
      const int groups = (N + 3) / 4;
      const dim3 grid((unsigned)(groups < cap2 ? groups : cap2));
      hipLaunchKernelGGL((gemv_pk_plain_kernel<2, 1, 2, 4>), grid, dim3(kGemvThreads), 0, st, m, N, K, x, y);
    } else {
      // whole passes over a grid that is resident at once: two workgroups per CU (a wave's half of x and the rows in flight take up to 230 registers)
      const bool c12 = ((K / 8 + 1) / 2 + 63) / 64 <= 12;
      const int groups = c12 ? (N + 3) / 4 : (N + 1) / 2;  // two rows per wave pair and pass / one
      const int passes = (groups + cap2 - 1) / cap2;
      const dim3 grid((unsigned)((groups + passes - 1) / passes));
      // 8192 < K <= 12288: either half of a row holds at least three whole pairs; 12288 < K <= 16384: at least five
      if (c12) hipLaunchKernelGGL((gemv_pk_halves_kernel<12, 2, 2, 3>), grid, dim3(kGemvThreads), 0, st, m, N, K, x, y);
      else hipLaunchKernelGGL((gemv_pk_halves_kernel<16, 1, 2, 5>), grid, dim3(kGemvThreads), 0, st, m, N, K, x, y);
    }
  }
  DL_CHECK_LAUNCH("dl_gemv_pk");
  return DL_OK;
}
