// x3p_stream.hip -- the row streams of the packed GEMM (gemm_x3p.h
// gemm_x3p_bwd_stream): one persistent launch beside a running recurrence
// packs its rows as they appear and multiplies them per direction, on 128
// tiles (x3p_bwd_stream_kernel, tile: x3p_tile128.h) or 256 tiles
// (x3p_bwd_stream256_kernel, k loop: x3p_tile256.h); and their self-test.
#include <vector>

#include "x3p_tile128.h"
#include "x3p_tile256.h"

namespace kctc {
namespace {

// ---- backward stream: pack jobs + GEMM jobs in one persistent launch ----
// Rows of direction d of a backward recurrence's dGates (E) become available
// step by step (direction 0 from t = T-1 down, direction 1 from t = 0 up).
// Per (row tile, direction) slot: P pack jobs (rows -> packed hi/lo with a
// per-row exponent, sc1 stores, then done[d][rt] += 1) and gx GEMM jobs
// (wait done == P, then the tile with sc1 LDS-DMA, combine epilogue).  Slots
// alternate directions in production order; jobs are taken from one counter,
// so a GEMM job only ever waits for pack jobs that running blocks own.
template <int KW, bool BFM, int NWV = 4>
__device__ __forceinline__ void bwd_pack_rows(const PParams &p, int d, int r0, int r1) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int K = p.KB * (BFM ? 64 : 32);
  for (int r = r0 + w; r < r1; r += NWV) {
    const auto rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.E + (long)r * p.lde + d * p.edoff), 0,
                                                      K * 4, 0x00020000);
    floatx4 v[KW];
    float mx = 0.f;
#pragma unroll
    for (int i = 0; i < KW; i++) {
      const int k = 4 * lane + 256 * i;
      v[i] = floatx4{0.f, 0.f, 0.f, 0.f};
      if (k < K) v[i] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(rx, k * 4, 0, 16));
      mx = fmaxf(mx, fmaxf(fmaxf(fabsf(v[i][0]), fabsf(v[i][1])), fmaxf(fabsf(v[i][2]), fabsf(v[i][3]))));
    }
    const auto ro = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16 *>(p.A) + (long)d * p.sA + (long)r * p.KB * 64, 0, p.KB * 128,
                                                      0x00020000);
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    if constexpr (BFM) {  // bf16 rows [KB][64], no exponent
#pragma unroll
      for (int i = 0; i < KW; i++) {
        const int k = 4 * lane + 256 * i;
        if (k < K) {
          bf16x4 h;
#pragma unroll
          for (int j = 0; j < 4; j++) h[j] = (__bf16)v[i][j];
          __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, h), ro, k * 2, 0, 16);
        }
      }
      continue;
    }
    mx = wave_max_l63(mx);
    const int e = split_exp_d(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(mx), 63)));
#pragma unroll
    for (int i = 0; i < KW; i++) {
      const int k = 4 * lane + 256 * i;
      if (k < K) {
        halfx4 h, l;
        split4(v[i], e, h, l);
        const int kb = k >> 5, off = k & 31;
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, h), ro, (kb * 64 + off) * 2, 0, 16);
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, l), ro, (kb * 64 + 32 + off) * 2, 0, 16);
      }
    }
    if (lane == 0)
      __hip_atomic_store(const_cast<int *>(p.eA) + (long)d * p.seA + r, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <int KW, bool BFM>
__global__ __launch_bounds__(NTH, 2) void x3p_bwd_stream_kernel(PParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  int *next = reinterpret_cast<int *>(lds + 2 * 2 * TILEB);
  int *seen = next + 1;  // [2] producer epochs seen
  int *bc = next + 3;    // combine broadcast
  if (threadIdx.x == 0) { seen[0] = 0; seen[1] = 0; }
  const int J = p.P + p.gx, total = 2 * p.nrt * J, rows_per = TB / p.P;
  if (on_pinned_xcd(p, bc)) return;  // before taking any job
  while (true) {
    const int id = next_job(p.counter, next);
    if (id >= total) break;
    const int slot = id / J, r = id - slot * J, d = slot & 1, rank = slot >> 1;
    const int rt = d == 0 ? p.nrt - 1 - rank : rank;
    if (r < p.P) {
      const int ra = rt * TB + r * rows_per, rb = min(p.M, ra + rows_per);
      if (ra < rb) {
        // E rows of step s are stored one step later: complete at epoch s + 3
        // (s = steps done before it; the last step gets epoch T + 2 at exit)
        const int ta = ra / p.sN, tb = (rb - 1) / p.sN;
        wait_epoch(p, d, d == 0 ? p.sT + 2 - ta : tb + 3, seen);
        bwd_pack_rows<KW, BFM>(p, d, ra, rb);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (threadIdx.x == 0) __hip_atomic_fetch_add(p.done + d * p.nrt + rt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      // a barrier after the lane-0 atomic: with the atomic as the last thing
      // in the body hipcc structured the job loop as divergent (the loop latch
      // masks lanes off), which left lane 0 of wave 0 behind with the
      // barriers inside the loop still completing for the rest
      __syncthreads();
    } else {
      wait_count(p.done + d * p.nrt + rt, p.P, p.serr);
      x3p_tile<2, BFM>(p, lds, rt, r - p.P, d, 0, bc);
      __syncthreads();
    }
  }
}

// ---- the backward stream on 256 x 256 tiles ------------------------------
// x3p_bwd_stream_kernel's job list at the p256 tile (512 threads, 128 KB
// LDS, one block per CU): per (row tile, direction) slot P pack jobs of
// 256 / P rows (8 waves) and gx GEMM jobs of 256 x 256 over the direction's
// whole K, A by sc1 LDS-DMA (rows packed by other CUs during this launch).
// A 256 x 256 tile issues 2x the MFMAs per LDS byte of the 128 tile, so the
// dx GEMM keeps up with the recurrence on about a third of the CUs the 128
// version needed, and the rest run the weight GEMMs (gemm_x3p avoid_word).
// The two directions' partials meet in the accumulator layout
// (part + tile * 256 * 256: thread t's (i, j) fragment is 16 B at
// [i * 4 + j][t]): the first to arrive stores its partial (sc1), the second
// adds it and writes C -- part0 + part1 either way round.
// ks / S: this job's K-split of S (S > 1: a tail slot, its tile's partials
// meet in part2)
template <bool BFM>
__device__ __forceinline__ void p256_bwd_tile(const PParams &p, unsigned char *lds, int tm, int tn, int d, int *bc,
                                              int ks, int S) {
  const _Float16 *A = p.A + (long)d * p.sA, *B = p.B + (long)d * p.sB;
  const int m0 = tm * TB2, n0 = tn * TB2;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wm = (wid >> 2) * 128, wn = (wid & 3) * 64;
  const int fr = lane & 15, fq = lane >> 4;
  floatx4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
  const int kbs = (p.KB + S - 1) / S, kb0 = ks * kbs, nk = max(0, min(p.KB, kb0 + kbs) - kb0);
  // transposed accumulators (p256_row TR): lane (fr, fq) holds row
  // m0 + wm + 16 i + fr, columns n0 + wn + 16 j + 4 fq .. + 3 of C
  if (nk > 0) p256_kloop_spread<BFM, 16, true>(A, B, p.M, p.N, p.KB, m0, n0, kb0, nk, lds, wm, wn, fr, fq, acc);
  if constexpr (!BFM) {  // to values: 2^-(eA[row] + eB[col]) (eA written by other CUs: sc1 loads)
    const int *eA = p.eA + (long)d * p.seA, *eB = p.eB + (long)d * p.seB;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      int eb[4];
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const int col = n0 + wn + j * 16 + fq * 4 + c;
        eb[c] = col < p.N ? eB[col] : 0;
      }
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const int row = m0 + wm + i * 16 + fr;
        const int ea = row < p.M ? __hip_atomic_load(eA + row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
#pragma unroll
        for (int c = 0; c < 4; c++) acc[i][j][c] = ldexpf(acc[i][j][c], -(ea + eb[c]));
      }
    }
  }
  // C row piece (i, j) of this lane: + bias + bias2 of each column (gemm_x3p's
  // order), one 16-B store where the piece is whole and aligned
  const bool vec = ((reinterpret_cast<unsigned long>(p.C) & 15) | (p.ldc & 3)) == 0;
  // the biases of this lane's 16 columns (a column's only: computed once)
  float bsum[4][4];
  if (p.bias) {
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const int col = min(n0 + wn + j * 16 + fq * 4 + c, p.N - 1);
        const long bo = (long)(col / p.bcols) * p.sBias + col % p.bcols;
        float badd = 0.f;
        badd += p.bias[bo];
        if (p.bias2) badd += p.bias2[bo];
        bsum[j][c] = badd;
      }
  }
  auto put = [&](int i, int j, floatx4 v) {
    const int row = m0 + wm + i * 16 + fr, col0 = n0 + wn + j * 16 + fq * 4;
    if (row >= p.M || col0 >= p.N) return;
    if (p.bias) {
#pragma unroll
      for (int c = 0; c < 4; c++) v[c] = v[c] + bsum[j][c];
    }
    float *o = p.C + (long)row * p.ldc + col0;
    if (vec && col0 + 3 < p.N) {
      *reinterpret_cast<floatx4 *>(o) = v;
    } else {
#pragma unroll
      for (int c = 0; c < 4; c++)
        if (col0 + c < p.N) o[c] = v[c];
    }
  };
  const long tile = (long)tm * p.gx + tn;
  int *arr = p.arrive + tile;
  // a tail tile (one of its directions split p.tails ways): every partial
  // goes to its slot q of [other direction's, split 0 .. tails - 1] in
  // part2, then arrives; the last arrival adds the slots up in q order (acc
  // is dead after the store: the tail costs the k loop no registers)
  const bool tail = p.tailr > 0 && (tm < p.tailr || tm >= p.nrt - p.tailr);
  if (tail) {
    const int n = p.tails + 1, q = S > 1 ? 1 + ks : 0;
    const int ti = tm < p.tailr ? tm : p.tailr + tm - (p.nrt - p.tailr);
    float *base = p.part2 + ((long)(ti * p.gx + tn) * n) * (TB2 * TB2);
    {
      const auto rq = __builtin_amdgcn_make_buffer_rsrc(base + (long)q * (TB2 * TB2), 0, TB2 * TB2 * 4, 0x00020000);
#pragma unroll
      for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = 0; j < 4; j++)
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[i][j]), rq,
                                                 ((i * 4 + j) * NTH2 + (int)threadIdx.x) * 16, 0, 16);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) *bc = __hip_atomic_fetch_add(arr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (__builtin_amdgcn_readfirstlane(*bc) == n - 1) {
      const auto rb = __builtin_amdgcn_make_buffer_rsrc(base, 0, n * TB2 * TB2 * 4, 0x00020000);
      for (int i = 0; i < 8; i++)
        for (int j = 0; j < 4; j++) {
          const int off = ((i * 4 + j) * NTH2 + (int)threadIdx.x) * 16;
          floatx4 v = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(rb, off, 0, 16));
          for (int qq = 1; qq < n; qq++)
            v += __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(rb, off + qq * TB2 * TB2 * 4, 0, 16));
          put(i, j, v);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    return;
  }
  if (threadIdx.x == 0) *bc = __hip_atomic_fetch_add(arr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  const bool first = __builtin_amdgcn_readfirstlane(*bc) == 0;
  const auto rp = __builtin_amdgcn_make_buffer_rsrc(p.part + tile * (TB2 * TB2), 0, TB2 * TB2 * 4, 0x00020000);
  if (first) {
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
      for (int j = 0; j < 4; j++)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[i][j]), rp,
                                               ((i * 4 + j) * NTH2 + (int)threadIdx.x) * 16, 0, 16);
  } else {
    wait_count(arr, 4, p.serr);
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const floatx4 o = __builtin_bit_cast(
            floatx4, __builtin_amdgcn_raw_buffer_load_b128(rp, ((i * 4 + j) * NTH2 + (int)threadIdx.x) * 16, 0, 16));
        put(i, j, acc[i][j] + o);
      }
  }
  // unconditional barrier (see fwd_combine)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (first && threadIdx.x == 0) __hip_atomic_fetch_add(arr, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int KW, bool BFM>
__global__ __launch_bounds__(NTH2, 1) void x3p_bwd_stream256_kernel(PParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  int *next = reinterpret_cast<int *>(lds + 2 * 2 * TILEB2);
  int *seen = next + 1;  // [2] producer epochs seen
  int *bc = next + 3;    // combine broadcast
  if (threadIdx.x == 0) { seen[0] = 0; seen[1] = 0; }
  // slots of the regular ranks (P pack + gx GEMM jobs), then the tail ranks'
  // (P pack + gx x tails GEMM jobs)
  const int J0 = p.P + p.gx, J1 = p.P + p.gx * p.tails, nreg = 2 * (p.nrt - p.tailr);
  const int base1 = nreg * J0, total = base1 + 2 * p.tailr * J1, rows_per = TB2 / p.P;
  if (on_pinned_xcd(p, bc)) return;  // before taking any job
  while (true) {
    const int id = next_job(p.counter, next);
    if (id >= total) break;
    int slot, r;
    if (id < base1) {
      slot = id / J0;
      r = id - slot * J0;
    } else {
      slot = nreg + (id - base1) / J1;
      r = (id - base1) % J1;
    }
    const int d = slot & 1, rank = slot >> 1;
    // the producer's direction that walks the frames downwards takes the
    // row tiles from the last (a backward producer's direction 0, a forward
    // producer's direction 1)
    const bool down = (d == 0) != (p.fwdp != 0);
    const int rt = down ? p.nrt - 1 - rank : rank;
    if (r < p.P) {
      const int ra = rt * TB2 + r * rows_per, rb = min(p.M, ra + rows_per);
      if (ra < rb) {
        // E rows of step s are complete at epoch s + 3 (the last step's at T + 2)
        const int ta = ra / p.sN, tb = (rb - 1) / p.sN;
        wait_epoch(p, d, down ? p.sT + 2 - ta : tb + 3, seen);
        bwd_pack_rows<KW, BFM, NTH2 / 64>(p, d, ra, rb);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (threadIdx.x == 0) __hip_atomic_fetch_add(p.done + d * p.nrt + rt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __syncthreads();  // (see x3p_bwd_stream_kernel: reconverge after the lane-0 atomic)
    } else {
      wait_count(p.done + d * p.nrt + rt, p.P, p.serr);
      const int S = rank >= p.nrt - p.tailr ? p.tails : 1, gj = r - p.P;
      p256_bwd_tile<BFM>(p, lds, rt, gj % p.gx, d, bc, gj / p.gx, S);
      __syncthreads();
    }
  }
}

}  // namespace

size_t x3p_bwd_stream_ints(int M, int N) {
  const long nrt = ceil_div(M, TB), gx = ceil_div(N, TB);
  return (size_t)(1 + 2 * nrt + nrt * gx);
}

bool x3p_bwd_stream_256(int M, int N, int KB, bool bf16) {
  // per-tile buffer offsets stay below 2^31 (C rows are addressed as [M][ldc])
  return x3p_use_256(M, N) && KB * (bf16 ? 64 : 32) <= 4096;
}
// off by default: at configs[1] the streams end ~200 us after their
// producers with or without it (they run behind, not on the last jobs) and
// the extra partial traffic cost 1.4 % (752k vs 741k frames/s, same box)
int x3p_stream_tail_rows() { return 0; }
size_t x3p_bwd_stream_part2_floats(int N) {
  return (size_t)2 * x3p_stream_tail_rows() * ceil_div(N, TB2) * (kStreamTailSplit + 1) * TB2 * TB2;
}
size_t x3p_bwd_stream_part_floats(int M, int N) {
  return std::max((size_t)M * N, (size_t)ceil_div(M, TB2) * ceil_div(N, TB2) * TB2 * TB2);
}

void gemm_x3p_bwd_stream(hipStream_t s, const X3PBwdStream &a) {
  if (a.M <= 0 || a.N <= 0) return;
  if (!rnn_side_gated(s))
    throw std::logic_error("gemm_x3p_bwd_stream: streaming launch beside a recurrence without its residency gate");
  const int K = a.KB * (a.bf16 ? 64 : 32);
  if (K > 4096 || a.Nf <= 0 || (long)a.M * a.N * 4 >= (1L << 31) || (long)a.M * a.KB * 128 >= (1L << 31) ||
      (a.lde & 3) || (a.edoff & 3))
    throw std::invalid_argument("gemm_x3p_bwd_stream: unsupported shape");
  const bool t256 = x3p_bwd_stream_256(a.M, a.N, a.KB, a.bf16);
  if ((a.forward || a.bias) && !t256) throw std::invalid_argument("gemm_x3p_bwd_stream: forward producer needs 256 tiles");
  PParams p = x3p_problem(a.M, a.N, a.KB, t256 ? TB2 : TB, a.Ap, a.eA, a.B, a.eB, a.C, a.ldc, a.bias, a.bias2, a.sbias,
                          a.cnt,
                          {a.producer.lines, a.producer.nwg, a.T, a.Nf, a.rg, a.err, a.producer.xcd_word,
                           a.producer.xcd_count});
  p.sA = (long)a.M * a.KB * 64; p.seA = a.M; p.sB = a.sB; p.seB = a.seB;
  p.alpha = 1.f; p.beta = 0.f;
  p.batch = 2; p.split = 1; p.kbchunk = a.KB;
  p.E = a.E; p.lde = a.lde; p.edoff = a.edoff;
  p.P = 4;
  p.done = a.cnt + 1; p.arrive = a.cnt + 1 + 2 * p.nrt;  // within x3p_bwd_stream_ints (128-tile counts)
  p.part = a.part;
  p.fwdp = a.forward ? 1 : 0;
  p.bcols = a.bias_cols > 0 ? a.bias_cols : 1;
  KCTC_HIP_CHECK(hipMemsetAsync(a.cnt, 0, sizeof(int) * x3p_bwd_stream_ints(a.M, a.N), s));
  if (t256) {
    const int tr = a.tail_rows >= 0 ? a.tail_rows : x3p_stream_tail_rows();
    p.tailr = a.part2 && tr > 0 && p.nrt >= 2 * tr + 2 ? tr : 0;
    p.tails = p.tailr ? kStreamTailSplit : 1;
    p.part2 = a.part2;
  }
  // 128 tiles: tailr = 0, every slot has P pack and gx GEMM jobs
  const int total = 2 * (p.nrt - p.tailr) * (p.P + p.gx) + 2 * p.tailr * (p.P + p.gx * p.tails);
  const dim3 grid(std::min(total, a.producer.blocks > 0 ? a.producer.blocks : 96));
  x3p_with_kw<4>(K, [&](auto kw) {
    constexpr int KW = decltype(kw)::value;
    if (t256) {
      if (a.bf16) x3p_launch<x3p_bwd_stream256_kernel<KW, true>>(grid, NTH2, kLds256, s, p);
      else x3p_launch<x3p_bwd_stream256_kernel<KW, false>>(grid, NTH2, kLds256, s, p);
    } else {
      if (a.bf16) x3p_launch<x3p_bwd_stream_kernel<KW, true>>(grid, NTH, kLdsStream, s, p);
      else x3p_launch<x3p_bwd_stream_kernel<KW, false>>(grid, NTH, kLdsStream, s, p);
    }
  });
}

void x3p_row_stream_selftest(hipStream_t s, int M, int N, int KB, int forward, int tail_rows, const float *E,
                             const float *Wt, const float *bias, float *C) {
  const int K = KB * 32, Nf = 16, T = (M + Nf - 1) / Nf;
  if (M <= 0 || N <= 0 || KB <= 0 || M % Nf) throw std::invalid_argument("x3p_row_stream_selftest: shape");
  if (!x3p_bwd_stream_256(M, N, KB, false) && (forward || bias))
    throw std::invalid_argument("x3p_row_stream_selftest: a 128-tile shape takes a backward producer and no bias");
  const int tr = tail_rows >= 0 ? tail_rows : x3p_stream_tail_rows();
  const size_t ap = (size_t)2 * M * KB * 128, bp = (size_t)2 * N * KB * 128;
  const size_t part = sizeof(float) * x3p_bwd_stream_part_floats(M, N);
  const size_t part2 = sizeof(float) * (size_t)2 * tr * ceil_div(N, TB2) * (kStreamTailSplit + 1) * TB2 * TB2;
  const size_t cnt = sizeof(int) * x3p_bwd_stream_ints(M, N), fl = 4096;
  char *buf = nullptr;
  const size_t total = ap + bp + part + part2 + cnt + fl + sizeof(int) * 4 * (size_t)(M + N) + 4096;
  KCTC_HIP_CHECK(hipMalloc(&buf, total));
  char *o = buf;
  auto take = [&](size_t b) { char *r = o; o += (b + 255) / 256 * 256; return r; };
  _Float16 *A = reinterpret_cast<_Float16 *>(take(ap)), *B = reinterpret_cast<_Float16 *>(take(bp));
  float *pt = reinterpret_cast<float *>(take(part)), *pt2 = reinterpret_cast<float *>(take(part2));
  int *cn = reinterpret_cast<int *>(take(cnt));
  unsigned *flags = reinterpret_cast<unsigned *>(take(fl));
  int *eA = reinterpret_cast<int *>(take(sizeof(int) * 2 * (size_t)M)), *eB = reinterpret_cast<int *>(take(sizeof(int) * 2 * (size_t)N));
  // every epoch final: lines (d) at 32-word strides
  std::vector<unsigned> hf(fl / 4, (unsigned)(T + 2));
  hf[1000] = 0u;  // the error word
  KCTC_HIP_CHECK(hipMemcpyAsync(flags, hf.data(), fl, hipMemcpyHostToDevice, s));
  x3p_pack_rows(s, Wt, K, N, K, B, eB, 0.f, 2, (long)N * K, (long)N * KB * 64, N);
  X3PBwdStream a;
  a.M = M; a.N = N; a.KB = KB;
  a.E = E; a.lde = 2L * K; a.edoff = K;
  a.Ap = A; a.eA = eA;
  a.B = B; a.eB = eB; a.sB = (long)N * KB * 64; a.seB = N;
  a.C = C; a.ldc = N;
  a.part = pt; a.part2 = tr > 0 ? pt2 : nullptr; a.tail_rows = tr; a.cnt = cn;
  a.producer.lines = flags; a.producer.nwg = 1; a.producer.blocks = 64;
  a.T = T; a.Nf = Nf; a.err = flags + 1000; a.rg = 1;
  a.forward = forward != 0;
  a.bias = bias; a.bias_cols = N;
  gemm_x3p_bwd_stream(s, a);
  KCTC_HIP_CHECK(hipStreamSynchronize(s));
  unsigned err = 0;
  KCTC_HIP_CHECK(hipMemcpy(&err, flags + 1000, sizeof(unsigned), hipMemcpyDeviceToHost));
  KCTC_HIP_CHECK(hipFree(buf));
  if (err) throw std::runtime_error("x3p_row_stream_selftest: wait timeout");
}

}  // namespace kctc
