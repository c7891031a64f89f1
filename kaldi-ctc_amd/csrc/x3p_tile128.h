// x3p_tile128.h -- one 128 x 128 tile of the packed GEMM (x3p_tile), private
// to x3p_gemm.hip (plain and forward image-stream jobs) and x3p_stream.hip
// (the 128-tile row stream's GEMM jobs).
//
// A plain fp16 matrix-core tile: 4 waves (2 x 2, 64 x 64 each, 16
// v_mfma_f32_16x16x32_f16 accumulators), one 32-k block per stage.  Stages
// are filled by LDS-DMA into the swizzled image of x3p_common.h, or from
// registers where the rows were just written by other CUs.  Two stages in
// flight, one barrier per stage.
#pragma once
#include "x3p_common.h"

namespace kctc {
namespace {

// streaming A operand: the producer's exchange images, read in place.  Step t
// of a bidirectional v6 forward recurrence holds h_t * 2^14 as fp16 hi/lo
// A fragments, [kb = k / 32][hi | lo][16 rows n][32 k] halves (kb over both
// directions), sxs halves per step; packed row r = t * sN + n.  The tile image
// is the same swizzled one as issue_tile's, filled by sc1 register loads (the
// rows were just published by other CUs) + ds_write_b128.
__device__ __forceinline__ void load_tile_xch(const PParams &p, const _Float16 *__restrict__ X, int r0, int kb,
                                              u32x4 (&reg)[4]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16 *>(X), 0, 0x7fffffff, 0x00020000);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int r = (w * 4 + i) * 8 + (lane >> 3);
    const int c = (lane & 7) ^ (r & 7);
    const int gr = min(r0 + r, p.M - 1);
    const int t = gr / p.sN, n = gr - t * p.sN;
    const long off = (long)t * p.sxs + (long)(n >> p.sgsh) * p.sxg +
                     (((long)kb * 2 + (c >> 2)) * 16 + (n & ((1 << p.sgsh) - 1))) * 32 +
                     (c & 3) * 8;
    reg[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(off * 2), 0, 16 /* sc1 */);
  }
}
// the packed layout [row][KB][64], rows written by other workgroups (sc1 stores):
// sc1 loads to registers, the tile image as issue_tile's
__device__ __forceinline__ void load_tile_sc1(const _Float16 *__restrict__ P, int rows, int r0, int KB, int kb,
                                              u32x4 (&reg)[4]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int r = (w * 4 + i) * 8 + (lane >> 3);
    const int c = (lane & 7) ^ (r & 7);
    const int gr = min(r0 + r, rows - 1);
    // one (uniform) descriptor: the host keeps rows * KB * 128 B below 2^31
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16 *>(P), 0, 0x7fffffff, 0x00020000);
    reg[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(((long)gr * KB + kb) * 128 + c * 16), 0, 16 /* sc1 */);
  }
}
__device__ __forceinline__ void store_tile_lds(unsigned char *dst, const u32x4 (&reg)[4]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 4; i++) *reinterpret_cast<u32x4 *>(dst + (w * 4 + i) * 1024 + lane * 16) = reg[i];
}

// (Inside the polling loops every branch is wave-uniform; the single-lane
// stores of the outcome come after the loop: a lane-0 store in front of a
// `break` let the compiler leave lane 0 of wave 0 switched off, observed as
// EXEC = ...fffe and a workgroup running on without its thread 0.)
__device__ void x3p_wait_rows(const PParams &p, int m0, int *prog, int pd) {
  // prog[0..1]: steps known published by directions 0 / 1 (LDS cache; every
  // wave reads it before the barrier, wave 0 writes it only after).
  // pd = 0 / 1: only that producer direction's rows are needed (-1: both)
  const int r1 = min(p.M, m0 + TB) - 1;
  const int t0 = m0 / p.sN, t1 = r1 / p.sN;
  const int need0 = pd == 1 ? -1 : t1, need1 = pd == 0 ? -1 : p.sT - 1 - t0;
  const bool ok = __builtin_amdgcn_readfirstlane(prog[0] >= need0 && prog[1] >= need1);
  __syncthreads();
  if (ok) return;
  if (wave_id() == 0) {
    const unsigned long long ts = __builtin_amdgcn_s_memrealtime();
    int s0 = 0, s1 = 0, spins = 0;
    bool failed = false;
    while (true) {
      // epochs: step + 2; the slowest row group decides ([group][dir][wg] lines)
      s0 = s1 = 1 << 30;
      for (int gi = 0; gi < p.srg; gi++) {
        s0 = min(s0, (int)wave_flags_min(p.sflags + 32L * (2 * gi) * p.snwg, p.snwg) - 2);
        s1 = min(s1, (int)wave_flags_min(p.sflags + 32L * (2 * gi + 1) * p.snwg, p.snwg) - 2);
      }
      if (s0 >= need0 && s1 >= need1) break;
      failed = wave_timed_out(p.serr, spins++, ts, 0);
      if (failed) break;  // the producer stopped: flag it, finish on whatever is there
      backoff(max(need0 - s0, need1 - s1));
    }
    if (failed) s0 = s1 = 1 << 30;
    if (threadIdx.x == 0) { prog[0] = s0; prog[1] = s1; }
    if (failed) wave_fail(p.serr);
  }
  __syncthreads();
}

// the two directions' partial products of output tile (tm, tn) meet here:
// the first to arrive publishes its partial (sc1), the second adds it and
// writes C.  dx = part0 + part1 either way (fp addition commutes), so the
// result does not depend on the order of arrival.
__device__ __forceinline__ void bwd_combine(const PParams &p, floatx4 (&acc)[4][4], const int (&ea)[4][4], const int (&eb)[4],
                            int tm, int tn, int m0, int n0, int wm, int wn, int fr, int fq, int *bc) {
  int *arr = p.arrive + (long)tm * p.gx + tn;
  if (threadIdx.x == 0) *bc = __hip_atomic_fetch_add(arr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  const bool first = __builtin_amdgcn_readfirstlane(*bc) == 0;
  const auto rp = __builtin_amdgcn_make_buffer_rsrc(p.part, 0, 0x7fffffff, 0x00020000);
  if (!first) wait_count(arr, 4, p.serr);
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int col = n0 + wn + j * 16 + fr;
      if (col >= p.N) continue;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = m0 + wm + i * 16 + fq * 4 + r;
        if (row >= p.M) continue;
        const float v = ldexpf(acc[i][j][r], -(ea[i][r] + eb[j]));
        const int off = (int)(((long)row * p.N + col) * 4);
        if (first) {
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rp, off, 0, 16);
        } else {
          const float o = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rp, off, 0, 16));
          p.C[(long)row * p.ldc + col] = v + o;
        }
      }
    }
  // unconditional barrier (see fwd_combine)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (first && threadIdx.x == 0) __hip_atomic_fetch_add(arr, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Direction-split streaming (p.sdir): the K of the projection is [h_fwd |
// h_bwd], and the forward half of frame t is ready at producer step t, the
// backward half at step T-1-t -- so each C tile is two half-K jobs, taken in
// the order their rows appear (forward half: row tiles ascending, backward
// half: descending), and the work is spread over the whole recurrence instead
// of its second half.  The halves meet in C: the first to arrive stores its
// partial (sc1), the second adds it, its own and the bias and writes C.
// (v0 + v1) + bias is the same either way round, so C does not depend on the
// order of arrival.
__device__ __forceinline__ void fwd_combine(const PParams &p, floatx4 (&acc)[4][4], const int (&ea)[4][4],
                                            const int (&eb)[4], int tm, int tn, int b, int m0, int n0, int wm, int wn,
                                            int fr, int fq, int *bc) {
  const long tile = ((long)tm * p.batch + b) * p.gx + tn;
  int *arr = p.arrive + tile;
  if (threadIdx.x == 0) *bc = __hip_atomic_fetch_add(arr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  const bool first = __builtin_amdgcn_readfirstlane(*bc) == 0;
  // the partial travels in the accumulator layout: thread t's (i, j) fragment
  // is 16 B at [tile][i * 4 + j][t], so both halves store / load whole,
  // coalesced 16-B chunks (sc1: the other half may run on another XCD)
  const auto rp = __builtin_amdgcn_make_buffer_rsrc(p.part + tile * (TB * TB), 0, TB * TB * 4, 0x00020000);
  floatx4 v[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int r = 0; r < 4; r++) v[i][j][r] = ldexpf(acc[i][j][r], -(ea[i][r] + eb[j]));
  if (first) {
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v[i][j]), rp,
                                               ((i * 4 + j) * NTH + (int)threadIdx.x) * 16, 0, 16);
  } else {
    wait_count(arr, 4, p.serr);
    float *C = p.C + (long)b * p.sC;
    const float *bias = p.bias ? p.bias + (long)b * p.sBias : nullptr;
    const float *bias2 = p.bias2 ? p.bias2 + (long)b * p.sBias : nullptr;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const floatx4 o = __builtin_bit_cast(
            floatx4, __builtin_amdgcn_raw_buffer_load_b128(rp, ((i * 4 + j) * NTH + (int)threadIdx.x) * 16, 0, 16));
        const int col = n0 + wn + j * 16 + fr;
        if (col >= p.N) continue;
        float badd = 0.f;
        if (bias) badd += bias[col];
        if (bias2) badd += bias2[col];
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int row = m0 + wm + i * 16 + fq * 4 + r;
          if (row < p.M) C[(long)row * p.ldc + col] = (v[i][j][r] + o[r]) + badd;
        }
      }
  }
  // the barrier is unconditional: under `if (first)` (as bwd_combine had it)
  // the compiler let waves of this inlined copy skip it (observed: a hang)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (first && threadIdx.x == 0) __hip_atomic_fetch_add(arr, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// SM (source mode): 0 packed A via LDS-DMA; 1 A = a forward producer's
// exchange images (sc1 register loads); 2 packed A just written by other CUs
// (LDS-DMA with sc1, exponents read with sc1) and the two-direction combine
// epilogue of the backward stream.
// BFM: the operands are bf16-packed ([row][KB][64] bf16, 64 consecutive k per
// 128-B block): a stage is two v_mfma_f32_16x16x32_bf16 (chunks fq and 4 + fq)
// instead of the three split-fp16 products, no exponents.
// one k block of MFMAs on the LDS stage `cur` (A and B tiles)
template <bool BFM>
__device__ __forceinline__ void x3p_kblock(const unsigned char *cur, int wm, int wn, int fr, int fq,
                                           floatx4 (&acc)[4][4]) {
  halfx8 ah[4], al[4], bh[4], bl[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    ah[i] = frag(cur, wm + i * 16 + fr, fq);
    al[i] = frag(cur, wm + i * 16 + fr, 4 + fq);
  }
#pragma unroll
  for (int j = 0; j < 4; j++) {
    bh[j] = frag(cur + TILEB, wn + j * 16 + fr, fq);
    bl[j] = frag(cur + TILEB, wn + j * 16 + fr, 4 + fq);
  }
  if constexpr (BFM) {
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ah[i]),
                                                            __builtin_bit_cast(bf16x8, bh[j]), acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, al[i]),
                                                            __builtin_bit_cast(bf16x8, bl[j]), acc[i][j], 0, 0, 0);
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bl[j], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[i], bh[j], acc[i][j], 0, 0, 0);
  }
}

// k loop of the register-loaded A modes (SM 1: a forward producer's images,
// SM 2: rows packed by other workgroups; both sc1 loads whose latency is a
// MALL / other-XCD round trip): A is prefetched TWO k blocks ahead in a
// two-slot register ring (the loop is unrolled by two so the ring indices are
// static), B by LDS-DMA one block ahead, and the stage hand-over waits with a
// counted vmcnt that leaves the newest A prefetch in flight plus a raw
// s_barrier (a __syncthreads() would drain it).  Issue order per block it:
// B(it + 1) then A(it + 2), so vmcnt(4) at the end of block it means B(it + 1)
// and A(it + 1) have landed.  The body is straight-line (the loads past the
// last block re-read it, clamped, and are drained after the loop): with the
// loads under branches the compiler put a vmcnt(0) in front of every
// prefetch.  Even block counts only (the caller falls back otherwise).
template <int SM, bool BFM>
__device__ __forceinline__ void x3p_kloop_reg(const PParams &p, unsigned char *lds, const _Float16 *A,
                                              const _Float16 *B, int m0, int n0, int kb0, int nk, int wm, int wn,
                                              int fr, int fq, floatx4 (&acc)[4][4]) {
  u32x4 r0[4], r1[4];
  const int kbl = kb0 + nk - 1;
  auto loadA = [&](int kb, u32x4 (&r)[4]) {
    if constexpr (SM == 1) load_tile_xch(p, A, m0, min(kb, kbl), r);
    else load_tile_sc1(A, p.M, m0, p.KB, min(kb, kbl), r);
  };
  auto stage_wait = [&]() {
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };
  loadA(kb0, r0);
  issue_tile(B, p.N, n0, p.KB, kb0, lds + TILEB);
  loadA(kb0 + 1, r1);
  store_tile_lds(lds, r0);
  stage_wait();
  // block it: cur holds A(it), B(it); rn holds A(it + 1); rf is free
  auto body = [&](int it, u32x4 (&rf)[4], u32x4 (&rn)[4]) {
    unsigned char *cur = lds + (it & 1) * 2 * TILEB;
    unsigned char *nxt = lds + ((it + 1) & 1) * 2 * TILEB;
    issue_tile(B, p.N, n0, p.KB, min(kb0 + it + 1, kbl), nxt + TILEB);
    loadA(kb0 + it + 2, rf);
    x3p_kblock<BFM>(cur, wm, wn, fr, fq, acc);
    store_tile_lds(nxt, rn);
    stage_wait();
  };
  for (int it = 0; it < nk; it += 2) {
    body(it, r0, r1);
    body(it + 1, r1, r0);
  }
  // the clamped loads past the last block land before anyone reuses the stages
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

template <int SM, bool BFM = false>
__device__ __forceinline__ void x3p_tile(const PParams &p, unsigned char *lds, int tm, int tn, int b, int ks, int *prog) {
  constexpr bool STREAM = SM == 1;
  const _Float16 *A = p.A + (long)b * p.sA;
  const _Float16 *B = p.B + (long)b * p.sB;
  const int m0 = tm * TB, n0 = tn * TB;
  const int kb0 = ks * p.kbchunk, kb1 = min(p.KB, kb0 + p.kbchunk);
  const int nk = kb1 > kb0 ? kb1 - kb0 : 0;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wm = (wid >> 1) * 64, wn = (wid & 1) * 64;
  const int fr = lane & 15, fq = lane >> 4;

  floatx4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

  if (STREAM) x3p_wait_rows(p, m0, prog, p.sdir ? ks : -1);
  if constexpr (SM != 0) {
    if (nk >= 2 && !(nk & 1)) {
      x3p_kloop_reg<SM, BFM>(p, lds, A, B, m0, n0, kb0, nk, wm, wn, fr, fq, acc);
      goto epilogue;
    }
  }
  {
  // LDS: [2 stages][A tile | B tile]
  u32x4 ra[4];
  if (nk > 0) {
    if (STREAM) {
      load_tile_xch(p, A, m0, kb0, ra);
      store_tile_lds(lds, ra);
    } else if (SM == 2) {  // rows packed by other workgroups: sc1 loads to registers (not LDS-DMA)
      load_tile_sc1(A, p.M, m0, p.KB, kb0, ra);
      store_tile_lds(lds, ra);
    } else {
      issue_tile(A, p.M, m0, p.KB, kb0, lds);
    }
    issue_tile(B, p.N, n0, p.KB, kb0, lds + TILEB);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int it = 0; it < nk; it++) {
    unsigned char *cur = lds + (it & 1) * 2 * TILEB;
    unsigned char *nxt = lds + ((it + 1) & 1) * 2 * TILEB;
    if (it + 1 < nk) {
      if (STREAM) load_tile_xch(p, A, m0, kb0 + it + 1, ra);
      else if (SM == 2) load_tile_sc1(A, p.M, m0, p.KB, kb0 + it + 1, ra);
      else issue_tile(A, p.M, m0, p.KB, kb0 + it + 1, nxt);
      issue_tile(B, p.N, n0, p.KB, kb0 + it + 1, nxt + TILEB);
    }
    x3p_kblock<BFM>(cur, wm, wn, fr, fq, acc);
    if ((STREAM || SM == 2) && it + 1 < nk) store_tile_lds(nxt, ra);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  }
epilogue:

  // epilogue: acc[i][j][r] -> C[m0+wm+16i+4fq+r][n0+wn+16j+fr], times 2^-(eA + eB)
  const int *eA = p.eA ? p.eA + (long)b * p.seA : nullptr;
  const int *eB = p.eB ? p.eB + (long)b * p.seB : nullptr;
  int eb[4], ea[4][4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int col = n0 + wn + j * 16 + fr;
    eb[j] = col < p.N ? (p.eB ? eB[col] : p.eB0) : 0;
  }
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = m0 + wm + i * 16 + fq * 4 + r;
      ea[i][r] = row >= p.M || BFM ? 0
                 : SM == 2  ? __hip_atomic_load(eA + row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                 : p.eA     ? eA[row]
                            : p.eA0;
    }
  if (SM == 2) {
    bwd_combine(p, acc, ea, eb, tm, tn, m0, n0, wm, wn, fr, fq, prog);
    return;
  }
  if (STREAM && p.sdir) {
    fwd_combine(p, acc, ea, eb, tm, tn, b, m0, n0, wm, wn, fr, fq, prog + 2);
    return;
  }
  if (p.split > 1) {
    float *W = p.ws + ((long)ks * p.batch + b) * (long)p.M * p.N;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int col = n0 + wn + j * 16 + fr;
        if (col >= p.N) continue;
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int row = m0 + wm + i * 16 + fq * 4 + r;
          if (row < p.M) W[(long)row * p.N + col] = ldexpf(acc[i][j][r], -(ea[i][r] + eb[j]));
        }
      }
    return;
  }
  float *C = p.C + (long)b * p.sC;
  const float *bias = p.bias ? p.bias + (long)b * p.sBias : nullptr;
  const float *bias2 = p.bias2 ? p.bias2 + (long)b * p.sBias : nullptr;
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int col = n0 + wn + j * 16 + fr;
      if (col >= p.N) continue;
      float badd = 0.f;
      if (bias) badd += bias[col];
      if (bias2) badd += bias2[col];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = m0 + wm + i * 16 + fq * 4 + r;
        if (row < p.M) {
          float *c = C + (long)row * p.ldc + col;
          float v = p.alpha * ldexpf(acc[i][j][r], -(ea[i][r] + eb[j])) + badd;
          if (p.beta != 0.f) v += p.beta * *c;
          *c = v;
        }
      }
    }
}

}  // namespace
}  // namespace kctc
