// Stages of the bf16 / f16 prefill attention kernels (attn_prefill.hip), each written once.  The kernels there are compositions of these; what a kernel
// is for, and what was measured when it was added, is recorded above each kernel in attn_prefill.hip.
//
//   row preamble                       PfRow                                      every 16-bit kernel
//   tile kernels (mfma, keysplit; mfma_pipe keeps its own text and takes only its LDS layout from here, see its comment): K row-major and V^T in LDS, online softmax on the MFMA C layout (row = (lane>>4)*4 + reg, col = lane&15)
//     pf_load_q, pf_qk_tiles, pf_softmax_tiles, pf_pv_tiles, pf_write_vt4, pf_store_c_layout
//     (the four lines that store P between the softmax and pf_pv_tiles stay in each kernel: as a shared function the compiler hoists their 16 LDS addresses out of
//     the tile loop, and mfma<bf16, 64, causal, 2 waves> and mfma_pipe<bf16, 128, causal, 2 waves> each lose a wave of occupancy to it)
//   whole-row kernels (whole_d64, head_d64, whole_d128_causal): all keys of a head in LDS in matrix-core fragment order, softmax in registers
//     pf_stage_k_dma, pf_stage_vt_frag, pf_store_t_layout
//     (their key loops -- the `step` lambdas of whole_d64 and whole_d128_causal, the three-phase loop of head_d64 -- and the read side of the V^T swizzle stay in
//     the kernels: shared, whole_d128_causal measured 1.5-3 % slower)
//   PfTileLds / PfPipeLds / PfKeysplitLds / PfWholeLds: the LDS layout of each family, read by the kernel (its indices) and by the launcher (its bytes)
#pragma once
#include <type_traits>

#include "dl_common.h"

namespace dl {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

template <typename T>
__device__ __forceinline__ f32x4_t mfma16(const uint4& a, const uint4& b, f32x4_t c);
template <>
__device__ __forceinline__ f32x4_t mfma16<bf16_t>(const uint4& a, const uint4& b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}
template <>
__device__ __forceinline__ f32x4_t mfma16<f16_t>(const uint4& a, const uint4& b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
}

// two fp32 -> one packed pair of the 16-bit type, round-to-nearest-even (bf16: v_cvt_pk_bf16_f32, the same bits as Elem<bf16_t>::from_f for finite values)
template <typename T>
__device__ __forceinline__ uint32_t pf_pack2(float a, float b) {
  if constexpr (Elem<T>::kBf16) {
    typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
    typedef float f2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f2{a, b}, bf2));
  } else {
    return (uint32_t)Elem<T>::from_f(a) | ((uint32_t)Elem<T>::from_f(b) << 16);
  }
}

constexpr int kBN = 64, kPad = 8;

// ---- LDS layouts (elements are 2 bytes) ----
// plain kernel: K [BN][LDK] | V^T [D][LDV] | P [NW][16][LDP]
template <int D, int NW, int BN>
struct PfTileLds {
  static constexpr int LDK = D + kPad, LDV = BN + kPad, LDP = BN + kPad;
  static constexpr int kTile = BN * LDK + D * LDV;  // elements of one K | V^T buffer
  static constexpr size_t kBytes = (size_t)(kTile + NW * 16 * LDP) * 2;
};
// pipelined kernel: two K | V^T buffers, then P
template <int D, int NW>
struct PfPipeLds : PfTileLds<D, NW, kBN> {
  static constexpr size_t kBytes = (size_t)(2 * PfTileLds<D, NW, kBN>::kTile + NW * 16 * PfTileLds<D, NW, kBN>::LDP) * 2;
};
// key-split kernel: K [NKEY][LDK] | V^T [D][LDV] (key pairs swizzled) | P [RW*KW][16][LDP]; after the last round the partials and the output rows alias them
template <int D, int RW, int KW>
struct PfKeysplitLds {
  static constexpr int NKEY = KW * kBN;  // keys per round
  static constexpr int LDK = D + kPad, LDV = NKEY + kPad, LDP = kBN + kPad, LDO = D + kPad;
  static constexpr int kPartF = ((D / 16) * 4 + 8) * 64;  // floats per partial: O[DT][4][64 lanes], m[4][64], l[4][64]
  static constexpr size_t kBytes = (size_t)(NKEY * LDK + D * LDV + RW * KW * 16 * LDP) * 2;
  static_assert(RW * (KW - 1) * kPartF * 4 + RW * 16 * LDO * 2 <= kBytes, "partials + output staging alias the tile buffers");
};
// whole-row kernels: K fragments [KT key tiles][D / 32 dim pieces][64 lanes][8] | V^T fragments [D / 16 dim tiles][KC 32-key chunks][64 lanes][8]; one fragment = 1 KiB
template <int D, int KT, int KC>
struct PfWholeLds {
  static_assert(KT == 2 * KC, "a 32-key chunk is two key tiles");
  static constexpr int kKT = KT, kKC = KC;  // key tiles, 32-key chunks: the most a row may hold
  static constexpr int PIECES = D / 32, DT = D / 16;
  static constexpr int kPartF = (2 + DT * 4) * 64;  // floats of one key range's published partial (whole_d64): m, l, O^T[DT][4], each [64 lanes]
  static constexpr int kKEl = KT * PIECES * 512;  // elements of the K region
  static constexpr size_t kKBytes = (size_t)kKEl * 2;
  static constexpr size_t kBytes = kKBytes + (size_t)DT * KC * 1024;
};
using PfWholeD64Lds = PfWholeLds<64, 38, 19>;   // up to 608 keys
using PfWholeD128Lds = PfWholeLds<128, 16, 8>;  // up to 256 keys

// ---- row preamble: where one (sequence, head)'s rows start ----
// K/V either come from the same packed projection output as q (fresh prefill: off = 0, Lk = L, constants to a kernel that only builds this form) or from the KV slab
// (chunk on a cache: keys [0, off) were cached before, this chunk's keys sit at [off, off + L); query j sees keys <= off + j)
template <int D>
struct PfRow {
  int tok0, L, off, Lk;
  int64_t kv_rs;
  const uint16_t *qb, *kb, *vb;
  // the row's extent first: a kernel leaves here when its block of query rows lies past L
  __device__ __forceinline__ PfRow(const int32_t* cu, int b) {
    tok0 = cu[b];
    L = cu[b + 1] - tok0;
  }
  __device__ __forceinline__ void bind(int h, int n_rep, const void* q_, const void* k_, const void* v_, int64_t q_rs, int64_t kv_rs_) {
    const int kvh = h / n_rep;
    qb = reinterpret_cast<const uint16_t*>(q_) + (int64_t)tok0 * q_rs + (int64_t)h * D;
    off = 0, Lk = L, kv_rs = kv_rs_;
    kb = reinterpret_cast<const uint16_t*>(k_) + (int64_t)tok0 * kv_rs + (int64_t)kvh * D;
    vb = reinterpret_cast<const uint16_t*>(v_) + (int64_t)tok0 * kv_rs + (int64_t)kvh * D;
  }
  __device__ __forceinline__ void bind(int b, int h, int n_rep, const void* q_, const void* k_, const void* v_, int64_t q_rs, int64_t kv_rs_,
                                       const int32_t* kv_len, int64_t kv_sb, int64_t kv_sh) {
    const int kvh = h / n_rep;
    qb = reinterpret_cast<const uint16_t*>(q_) + (int64_t)tok0 * q_rs + (int64_t)h * D;
    // (K and V rows sit at the same element offset of their tensors, in either form)
    const int64_t base = kv_len ? (int64_t)b * kv_sb + (int64_t)kvh * kv_sh : (int64_t)tok0 * kv_rs_ + (int64_t)kvh * D;
    off = kv_len ? kv_len[b] : 0;
    Lk = off + L;
    kv_rs = kv_len ? D : kv_rs_;
    kb = reinterpret_cast<const uint16_t*>(k_) + base;
    vb = reinterpret_cast<const uint16_t*>(v_) + base;
  }
};

// ======== tile kernels ========

// Q fragments (A operand): row = lane&15, k = (lane>>4)*8 .. +8; rows past L are zeros
template <int KS>
__device__ __forceinline__ void pf_load_q(uint4 (&qf)[KS], const uint16_t* qb, int qrow, int L, int64_t q_rs, int lg) {
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    qf[ks] = make_uint4(0, 0, 0, 0);
    if (qrow < L) qf[ks] = *reinterpret_cast<const uint4*>(qb + (int64_t)qrow * q_rs + ks * 32 + lg * 8);
  }
}

// the running (m, l, O) of a wave's 16 query rows, before the first key
template <int DT>
__device__ __forceinline__ void pf_init_state(f32x4_t (&acc_o)[DT], float (&m)[4], float (&l)[4]) {
#pragma unroll
  for (int i = 0; i < DT; ++i) acc_o[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
  }
}

// S = Q K^T over the NT 16-key tiles of a row-major K image (Ks: the first of the wave's NT * 16 key rows)
template <typename T, int KS, int NT, int LDK>
__device__ __forceinline__ void pf_qk_tiles(f32x4_t (&acc_s)[NT], const uint4 (&qf)[KS], const uint16_t* Ks, int lr, int lg) {
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    acc_s[nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const uint4 kf = *reinterpret_cast<const uint4*>(Ks + (nt * 16 + lr) * LDK + ks * 32 + lg * 8);
      acc_s[nt] = mfma16<T>(qf[ks], kf, acc_s[nt]);
    }
  }
}

// online softmax on the C layout: row = lg*4 + r (query qi0 + r), col = nt*16 + lr (key key0 + nt*16 + lr).  Scores become probabilities, (m, l) move on; the caller
// rescales its acc_o by alpha.
template <int NT, bool CAUSAL>
__device__ __forceinline__ void pf_softmax_tiles(f32x4_t (&acc_s)[NT], float (&m)[4], float (&l)[4], float (&alpha)[4], float scale, int key0, int qi0, int off, int Lk,
                                                 int lr) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qi = qi0 + r;
    float mx = -INFINITY;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int ki = key0 + nt * 16 + lr;
      float s = acc_s[nt][r] * scale;
      if (ki >= Lk || (CAUSAL && ki > qi + off)) s = -INFINITY;
      acc_s[nt][r] = s;
      mx = fmaxf(mx, s);
    }
    mx = row16_max(mx);
    const float mn = fmaxf(m[r], mx);
    const float ms = mn == -INFINITY ? 0.f : mn;
    alpha[r] = __expf(m[r] - ms);
    float rs = 0.f;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const float p = __expf(acc_s[nt][r] - ms);
      acc_s[nt][r] = p;
      rs += p;
    }
    rs = row16_sum(rs);
    l[r] = l[r] * alpha[r] + rs;
    m[r] = mn;
  }
}

template <int DT>
__device__ __forceinline__ void pf_rescale(f32x4_t (&acc_o)[DT], const float (&alpha)[4]) {
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc_o[dt][r] *= alpha[r];
}

// O += P V: P from the wave's 16 LDS rows Pw (written there in the C layout: Pw[(lg*4 + r) * LDP + nt*16 + lr]) in the A layout, vt_addr(dt, ks) = this lane's 16 bytes of V^T for dims dt*16 + lr, keys ks*32 + lg*8 .. +8 of the wave's tile
template <typename T, int DT, int KSTEPS, int LDP, typename VtAddr>
__device__ __forceinline__ void pf_pv_tiles(f32x4_t (&acc_o)[DT], const uint16_t* Pw, int lr, int lg, VtAddr vt_addr) {
#pragma unroll
  for (int ks = 0; ks < KSTEPS; ++ks) {
    const uint4 pf = *reinterpret_cast<const uint4*>(Pw + lr * LDP + ks * 32 + lg * 8);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const uint4 vf = *reinterpret_cast<const uint4*>(vt_addr(dt, ks));
      acc_o[dt] = mfma16<T>(pf, vf, acc_o[dt]);
    }
  }
}

// 4 keys x 8 dims (v[j] = 16 bytes of key j) -> dims 2e (lo) and 2e + 1 (hi) of the chunk, 4 keys each: one 8-byte write per dim
__device__ __forceinline__ void pf_transpose4(const uint4 (&v)[4], int e, uint2& lo, uint2& hi) {
  const uint32_t w0[4] = {v[0].x, v[0].y, v[0].z, v[0].w}, w1[4] = {v[1].x, v[1].y, v[1].z, v[1].w};
  const uint32_t w2[4] = {v[2].x, v[2].y, v[2].z, v[2].w}, w3[4] = {v[3].x, v[3].y, v[3].z, v[3].w};
  lo.x = (w0[e] & 0xffffu) | (w1[e] << 16);
  lo.y = (w2[e] & 0xffffu) | (w3[e] << 16);
  hi.x = (w0[e] >> 16) | (w1[e] & 0xffff0000u);
  hi.y = (w2[e] >> 16) | (w3[e] & 0xffff0000u);
}

// the same 4 keys x 8 dims into a row-major V^T image: dims ch*8 .. +8, keys at column col .. +4
template <int LDV>
__device__ __forceinline__ void pf_write_vt4(uint16_t* Vt, int ch, int col, const uint4 (&v)[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    uint2 lo, hi;
    pf_transpose4(v, e, lo, hi);
    *reinterpret_cast<uint2*>(Vt + (ch * 8 + 2 * e) * LDV + col) = lo;
    *reinterpret_cast<uint2*>(Vt + (ch * 8 + 2 * e + 1) * LDV + col) = hi;
  }
}

// epilogue of the C layout: acc_o * (1 / l) as 2-byte stores, rows qi0 .. qi0 + 3 of the sequence
template <typename T, int DT>
__device__ __forceinline__ void pf_store_c_layout(uint16_t* ob, int64_t out_rs, const f32x4_t (&acc_o)[DT], const float (&l)[4], int qi0, int L, int lr) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qi = qi0 + r;
    if (qi < L) {
      const float inv = l[r] > 0.f ? 1.0f / l[r] : 0.f;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) ob[(int64_t)qi * out_rs + dt * 16 + lr] = Elem<T>::from_f(acc_o[dt][r] * inv);
    }
  }
}

// ======== whole-row kernels ========

// K by LDS-DMA: one 1 KiB piece per (key tile, 32-dim piece), wave w takes the key tiles w, w + NWV, ..; all pieces of a key tile by the same wave, back to back (the
// later pieces' 128-byte lines are the first one's).  Keys past L are staged as copies of key L - 1.  The caller waits (s_waitcnt vmcnt(0)) before its barrier.
template <int PIECES, int NWV>
__device__ __forceinline__ void pf_stage_k_dma(unsigned char* smem, const uint16_t* kb, int64_t kv_rs, int L, int n_kt, int w, int lr, int lg) {
  typedef __attribute__((address_space(3))) unsigned char lds_u8;
  typedef __attribute__((address_space(1))) void glob_v;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_u8*)smem;
  for (int kt = w; kt < n_kt; kt += NWV) {
    int key = kt * 16 + lr;
    key = key < L ? key : L - 1;
#pragma unroll
    for (int ks = 0; ks < PIECES; ++ks) {
      const uint32_t voff = (uint32_t)key * (uint32_t)kv_rs * 2u + (uint32_t)(ks * 32 + lg * 8) * 2u;
      const uint32_t dst = __builtin_amdgcn_readfirstlane(lds0 + (uint32_t)(kt * PIECES + ks) * 1024u);
      uint32_t keep;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep)
                   : "v"(voff), "s"((const glob_v*)kb), "s"(dst)
                   : "memory");
    }
  }
}

// V through registers: 4 keys x 8 dims per task (1 << CH_BITS dim chunks per key quad) -> V^T fragments [dim tile][KC 32-key chunks][64 lanes][8], the 8-byte slot of key
// quad (h2, lg') in lane 16 lg' + dim.  Every load of the thread's (up to two per pass) tasks is requested before the first transpose: the staging is one memory round
// trip deep, not one per task.
template <int CH_BITS, int KC, int NT_>
__device__ __forceinline__ void pf_stage_vt_frag(uint16_t* Vf, const uint16_t* vb, int64_t kv_rs, int L, int n_kc, int tid) {
  constexpr int CH_MASK = (1 << CH_BITS) - 1;
  const int n_tasks = n_kc * (8 << CH_BITS);
  for (int t0 = tid; t0 < n_tasks; t0 += 2 * NT_) {
    uint4 vr[2][4];
    int tt[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int t = t0 + u * NT_;
      tt[u] = t < n_tasks ? t : t0;  // (a thread without a second task re-loads its first: unconditional loads, nothing is written twice)
      const int qd = tt[u] >> CH_BITS, ch = tt[u] & CH_MASK;
      const int kc = qd >> 3, h2 = (qd >> 2) & 1, lgf = qd & 3;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int key = kc * 32 + h2 * 16 + lgf * 4 + j;
        key = key < L ? key : L - 1;
        vr[u][j] = *reinterpret_cast<const uint4*>(vb + (int64_t)key * kv_rs + ch * 8);
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (u == 1 && t0 + NT_ >= n_tasks) break;
      const int qd = tt[u] >> CH_BITS, ch = tt[u] & CH_MASK;
      const int kc = qd >> 3, h2 = (qd >> 2) & 1, lgf = qd & 3;
      // Slot of dim `lrf` inside its 16-dim x 4-group fragment: 16 B per (group, dim), XOR-swizzled in the low three dim bits by (dim tile, dim bit 3).  Unswizzled, the
      // 64 lanes of one of these 8-byte writes (8 dim chunks x 8 key quads) all land on the same two bank pairs -- 32-way, 3 us of staging (first build); the swizzle is a
      // permutation inside each aligned 16-lane block, which keeps the consumers' ds_read_b128 conflict-free.  The readers undo it where they set up `vrd[dt]` (lr ^ (((dt << 1) | (lr >> 3)) & 7)).
      uint16_t* frag = Vf + ((ch >> 1) * KC + kc) * 512 + lgf * 16 * 8 + h2 * 4;
      const int swz = ((ch >> 1) << 1 | (ch & 1)) & 7, hi8 = (ch & 1) * 8;
#pragma unroll
      for (int e = 0; e < 4; ++e) {  // dims 2e, 2e + 1 of the chunk: 4 keys each -> one 8-byte write per dim
        uint2 lo, hi;
        pf_transpose4(vr[u], e, lo, hi);
        *reinterpret_cast<uint2*>(frag + (hi8 + ((2 * e) ^ swz)) * 8) = lo;
        *reinterpret_cast<uint2*>(frag + (hi8 + ((2 * e + 1) ^ swz)) * 8) = hi;
      }
    }
  }
}

// epilogue of the transposed layout (lane: query lr, dims dt*16 + lg*4 .. +4): acc_o * inv as 8-byte stores into the query's output row `ob`.
// PK: round pairs with pf_pack2 (whole_d128_causal); whole_d64 rounds each value with Elem<T>::from_f, as it always has (the two agree on finite values).
template <typename T, int DT, bool PK>
__device__ __forceinline__ void pf_store_t_layout(uint16_t* ob, const f32x4_t (&acc_o)[DT], float inv, int lg) {
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    uint2 o;
    if constexpr (PK) {
      o.x = pf_pack2<T>(acc_o[dt][0] * inv, acc_o[dt][1] * inv);
      o.y = pf_pack2<T>(acc_o[dt][2] * inv, acc_o[dt][3] * inv);
    } else {
      o.x = (uint32_t)Elem<T>::from_f(acc_o[dt][0] * inv) | ((uint32_t)Elem<T>::from_f(acc_o[dt][1] * inv) << 16);
      o.y = (uint32_t)Elem<T>::from_f(acc_o[dt][2] * inv) | ((uint32_t)Elem<T>::from_f(acc_o[dt][3] * inv) << 16);
    }
    *reinterpret_cast<uint2*>(ob + dt * 16 + lg * 4) = o;
  }
}

}  // namespace dl
