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
// The packed helpers (PkMat, pk_decode, pk_request_*, pk_pass_dot) and the add + rmsnorm body live in gemv_pk.h, which gemv.hip includes too.
#include "gemv_pk.h"

namespace dl {

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

// ---- plain prologue, long rows (down_proj; 8192 < K <= 16384), x in LDS: gemv_b1_plain_halves_kernel on packed rows at four workgroups per CU.  A row is
// shared by the two waves of a pair -- the row's two segments, split at the bf16 kernel's hv -- and the even wave adds the partial sums low half first.
// The workgroup stages x once as two zero-padded segment images of C chunk slots per lane each (image `half`: chunks [v0, v1) of x, then zeros: a read
// past the low half's end must not land on the high half's x), AFTER it has requested its first pass and headers, so that the staging shares the first
// weights' round trip.  A wave walks its segment in passes of SLOTS pairs inside a RUNTIME loop (when it is unrolled, the compiler hoists the LDS reads of x
// into registers and spills) with two pass buffers: the next pass of the rows is requested before the current one is dotted.  It dots all C chunk slots, the
// padded ones too, as the bf16 kernel does (a padded chunk adds +0, which is not nothing for a -0 accumulator).  R rows per pair and pass. ----
template <int R, int SLOTS>
__global__ __launch_bounds__(kGemvThreads) __attribute__((amdgpu_waves_per_eu(4, 4))) void gemv_pk_long_kernel(PkMat m, int N, int K, int C, const void* __restrict__ x_,
                                                                                                           void* __restrict__ y_) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4* xs = reinterpret_cast<uint4*>(smem);  // [2][64 C]
  __shared__ float part[R][kGemvThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // (a scalar: row addresses stay in SGPRs)
  const int half = wid & 1, pr = wid >> 1;
  const int nvec = K / 8;
  const int hv = ((nvec + 1) / 2 + 63) / 64 * 64;  // chunks of the low half (whole lane sets)
  const int v0 = half * hv, v1 = half ? nvec : (hv < nvec ? hv : nvec);
  const int nc = v1 - v0, nsp = (nc + 63) >> 6, nslots = C / 2;
  constexpr int RPW = R * kGemvThreads / 128;  // rows per workgroup pass
  const int groups = (N + RPW - 1) / RPW;
  auto row_of = [&](int grp, int r) {
    const int n = grp * RPW + pr * R + r;
    return n < N ? n : N - 1;
  };
  auto seg_of = [&](int grp, int r) { return m.data + (int64_t)row_of(grp, r) * m.row_bytes + (int64_t)v0 * 12; };
  // the weight stream starts BEFORE the staging: the headers of this workgroup's first rows and their first pass
  PkPass<R, SLOTS> pa, pb;
  uint2 hraw[R];
#pragma unroll
  for (int r = 0; r < R; ++r) hraw[r] = m.hdr[row_of((int)blockIdx.x, r)];
#pragma unroll
  for (int i = 0; i < SLOTS; ++i)
#pragma unroll
    for (int r = 0; r < R; ++r) pk_request_slot<true>(pa.lo[i][r], pa.nb[i][r], seg_of((int)blockIdx.x, r), nc, i, lane);
  {
    const uint4* x = reinterpret_cast<const uint4*>(x_);
    const int img = 64 * C, lo_end = hv < nvec ? hv : nvec;
    uint4 t[8];  // C <= 16: at most 2048 chunk slots, one round trip
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = tid + kGemvThreads * k;
      const int v = i < img ? i : hv + (i - img);
      const bool live = i < img ? v < lo_end : (i < 2 * img && v < nvec);
      t[k] = live ? x[v] : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = tid + kGemvThreads * k;
      if (i < 2 * img) xs[i] = t[k];
    }
  }
  __syncthreads();
  const uint4* xh = xs + half * 64 * C + lane;
  bool first = true;
  for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {
    const unsigned char* seg[R];
    PkHdr h[R];
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      seg[r] = seg_of(grp, r);
      h[r] = pk_uniform(hraw[r]);
      acc[r] = 0.f;
    }
    const int nxt = grp + (int)gridDim.x < groups ? grp + (int)gridDim.x : grp;
    auto request = [&](PkPass<R, SLOTS>& ps, int p0, bool slots) {
      if (slots) {
#pragma unroll
        for (int i = 0; i < SLOTS; ++i)
#pragma unroll
          for (int r = 0; r < R; ++r) pk_request_slot<true>(ps.lo[i][r], ps.nb[i][r], seg[r], nc, p0 + i, lane);
      }
      const int left = nsp - 2 * p0;  // (a pass of padding only has no span)
      pk_request_raw<R, SLOTS>(ps, m, h, (v0 >> 6) + 2 * p0, left > 0 ? left : 0, lane);
    };
    auto dot = [&](const PkPass<R, SLOTS>& ps, int p0) {
      pk_pass_dot<R, SLOTS>(m, ps, h, (v0 >> 6) + 2 * p0, nslots - p0, lane, acc, [&](int c) { return xh[64 * (2 * p0 + c)]; });
    };
    request(pa, 0, !first);  // (the workgroup's first pass is in flight since before the staging)
    first = false;
#pragma unroll
    for (int r = 0; r < R; ++r) hraw[r] = m.hdr[row_of(nxt, r)];  // the next rows' headers travel with this row's first pass
    for (int p0 = 0; p0 < nslots; p0 += 2 * SLOTS) {
      const bool hb = p0 + SLOTS < nslots;
      if (hb) request(pb, p0 + SLOTS, true);
      dot(pa, p0);
      if (hb) {
        if (p0 + 2 * SLOTS < nslots) request(pa, p0 + 2 * SLOTS, true);
        dot(pb, p0 + SLOTS);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      acc[r] = wave_sum(acc[r]);
      if (lane == 0 && half) part[r][wid] = acc[r];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int n = grp * RPW + pr * R + r;
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
  gemv_pk_body<PAIR, 2, 4, 2>(m, N, K, h_, h_out_, delta_, nw_, eps, y_, (int)blockIdx.x, (int)gridDim.x, nullptr, 0u);
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
  DL_REQUIRE(grid_cap >= 0, "dl_gemv_pk: bad grid_cap %d", grid_cap);
  PkMat m;
  if (const int rc = pk_mat_check("dl_gemv_pk", m, data, data_bytes, hdr, hdr_rows, pool, pool_spans, hb, N, K)) return rc;
  const int pro = mode & 3;
  const bool pair = (mode & DL_GEMV_OUT_SILU_PAIR) != 0;
  DL_REQUIRE((mode & ~(3 | DL_GEMV_OUT_SILU_PAIR)) == 0 && (pro == DL_GEMV_PLAIN || pro == DL_GEMV_ADDNORM), "dl_gemv_pk: bad mode %d", mode);
  DL_REQUIRE(!pair || (pro == DL_GEMV_ADDNORM && N % 2 == 0), "dl_gemv_pk: SILU_PAIR needs the ADDNORM prologue and an even N");
  if (grid_cap == 0) grid_cap = kPkGridCap;
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
    // (the x-in-registers launches run at most grid_cap / 2 workgroups, as dl_gemv's: two per CU, which leaves them 256 registers)
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
      // x in LDS: four workgroups per CU, so the grid is sized from the whole cap; whole passes over a grid that is resident at once.  C: the chunk slots
      // per lane of a segment that the bf16 kernel dots (12: either half holds at most 12 spans, else 16)
      const int C = ((K / 8 + 1) / 2 + 63) / 64 <= 12 ? 12 : 16;
      const int groups = (N + 1) / 2;  // one row per wave pair and pass
      const int passes = (groups + grid_cap - 1) / grid_cap;
      const dim3 grid((unsigned)((groups + passes - 1) / passes));
      hipLaunchKernelGGL((gemv_pk_long_kernel<1, 3>), grid, dim3(kGemvThreads), (size_t)2 * C * 1024, st, m, N, K, C, x, y);
    }
  }
  DL_CHECK_LAUNCH("dl_gemv_pk");
  return DL_OK;
}
