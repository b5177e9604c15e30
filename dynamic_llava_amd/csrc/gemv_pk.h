// The packed-row helpers and the add + rmsnorm streaming body of gemv_pk.hip, shared with the fused launches of gemv.hip (dl_gemv_qkv_attn_pk,
// dl_gemv_gu_tp_pk), which run the body as part of a wider grid.  The format: dynamic_llava_amd/bf16pack.py; the rules: the head of gemv_pk.hip.
#pragma once
#include "gemv_dot.h"
#include "gemv_prologue.h"
#include "granule.h"
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

// ---- add + rmsnorm prologue, x in LDS: gemv_body<bf16_t, 1, 1, PAIR, R, .> on packed rows, K % 1024 == 0 (whole pairs).  R rows per wave, up to SLOTS
// pairs of each in flight; the first PRE slots of the workgroup's first pass are requested before the prologue.  A device function with gemv_body's
// shape, so that the fused launches can run it as part of a wider grid: `bid` / `nblk` are this workgroup's index and the number of workgroups that
// share the rows; gran != nullptr: every output is ALSO published as an 8-byte {gtag, value bits} granule (granule.h).  A row's arithmetic does not
// depend on R, SLOTS or PRE. ----
template <bool PAIR, int R, int SLOTS, int PRE>
__device__ __forceinline__ void gemv_pk_body(const PkMat& m, int N, int K, const void* __restrict__ h_, void* __restrict__ h_out_, const void* __restrict__ delta_,
                                             const void* __restrict__ nw_, float eps, void* __restrict__ y_, const int bid, const int nblk, u64_t* gran, uint32_t gtag) {
  static_assert(!PAIR || R == 2, "a SiLU pair is two rows");
  static_assert(PRE <= SLOTS, "the early request is part of the first pass");
  using S = Elem<bf16_t>::storage;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  S* xs = reinterpret_cast<S*>(smem);  // [K]
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // (a scalar: row addresses stay in SGPRs)
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
#ifdef DL_QA_TIMING
    if (grp == bid && threadIdx.x == 0 && blockIdx.x < 1200) g_qa_stamps[blockIdx.x][2] = wall_clock64();
#endif
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = wave_sum(acc[r]);
    if (lane == 0) {
      if constexpr (PAIR) {
        if (n0 < n_out) store1<bf16_t>(y_, n0, gemv_silu_pair<bf16_t>(acc[0], acc[1]));
      } else {
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (n0 + r < N) {
            store1<bf16_t>(y_, n0 + r, acc[r]);
            if (gran) gr_store(gran + n0 + r, gtag, (uint32_t)Elem<bf16_t>::from_f(acc[r]));
          }
      }
    }
  }
}

// The host-side checks of a packed matrix for the add + rmsnorm body, shared by dl_gemv_pk and the fused entry points; fills `m`.
static inline int pk_mat_check(const char* who, PkMat& m, const void* data, int64_t data_bytes, const void* hdr, int64_t hdr_rows, const void* pool, int64_t pool_spans,
                               int hb, int N, int K) {
  DL_REQUIRE(data && hdr && pool, "%s: NULL pointer", who);
  DL_REQUIRE(N > 0 && K > 0 && K % 64 == 0 && K <= 16384, "%s: bad shape N=%d K=%d", who, N, K);
  DL_REQUIRE(hb >= 0 && hb <= 120, "%s: hb=%d is outside [0, 120]", who, hb);
  const int64_t row_bytes = (int64_t)K * 3 / 2;
  DL_REQUIRE(data_bytes >= (int64_t)N * row_bytes, "%s: %lld packed bytes, %d rows of K=%d need %lld", who, (long long)data_bytes, N, K, (long long)((int64_t)N * row_bytes));
  DL_REQUIRE(hdr_rows >= N, "%s: %lld row headers for %d rows", who, (long long)hdr_rows, N);
  DL_REQUIRE(pool_spans >= 1 && pool_spans < ((int64_t)1 << 31), "%s: the pool must hold at least one span (%lld)", who, (long long)pool_spans);
  DL_REQUIRE(((uintptr_t)data | (uintptr_t)pool) % 16 == 0 && (uintptr_t)hdr % 8 == 0, "%s: data / pool must be 16-byte aligned, hdr 8-byte", who);
  m.data = reinterpret_cast<const unsigned char*>(data);
  m.hdr = reinterpret_cast<const uint2*>(hdr);
  m.pool = reinterpret_cast<const unsigned char*>(pool);
  m.row_bytes = row_bytes;
  m.pool_last = (uint32_t)(pool_spans - 1);
  m.hb4 = (uint32_t)hb * 0x01010101u;
  return DL_OK;
}

}  // namespace dl
