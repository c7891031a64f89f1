// x3p_tile256.h -- the k loop of the 256 x 256 tile, private to x3p_gemm.hip
// (p256_tile) and x3p_stream.hip (p256_bwd_tile).
//
// ---- 256 x 256 tiles for the large GEMMs ----------------------------------
// Same packed operands and swizzled 128-B row images as x3p_tile, at 4x the
// tile area: 512 threads = 8 waves as 2 (M) x 4 (N), each wave a 128 x 64
// block of C (8 x 4 accumulators).  Per stage (one 128-B k block of both
// operands, 64 KB) a wave issues 96 split-fp16 (or 64 bf16) MFMAs against 24
// fragment reads, so the stage's LDS-DMA of the next block (8 x 16 B per
// thread) lands behind ~3000 SIMD cycles of matrix work; two stages (128 KB
// LDS), one workgroup per CU, one barrier per stage.  Tile ids are dealt to
// the XCDs in contiguous runs (decode_tile's remap) so that the blocks of an
// XCD share A and B panels in its L2.
#pragma once
#include "x3p_common.h"

namespace kctc {
namespace {

// one row block (16 rows of the wave's 128) of a k block: 4 (bf16: 2 x 4)
// or 12 (split-fp16) MFMAs against the wave's B fragments.  TR: operands
// swapped, the accumulators hold C^T (lane (fr, fq): row fr, columns
// 4 fq .. 4 fq + 3 of the 16 x 16 block -- 16-B row pieces for the epilogue)
template <bool BFM, bool TR = false>
__device__ __forceinline__ void p256_row(floatx4 (&acc)[4], halfx8 ah, halfx8 al, const halfx8 (&bh)[4],
                                         const halfx8 (&bl)[4]) {
  auto mm = [](halfx8 a, halfx8 b, floatx4 c) {
    if constexpr (BFM) {
      return TR ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, b), __builtin_bit_cast(bf16x8, a),
                                                          c, 0, 0, 0)
                : __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b),
                                                          c, 0, 0, 0);
    } else {
      return TR ? __builtin_amdgcn_mfma_f32_16x16x32_f16(b, a, c, 0, 0, 0)
                : __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
  };
  if constexpr (BFM) {
#pragma unroll
    for (int j = 0; j < 4; j++) acc[j] = mm(ah, bh[j], acc[j]);
#pragma unroll
    for (int j = 0; j < 4; j++) acc[j] = mm(al, bl[j], acc[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) acc[j] = mm(ah, bh[j], acc[j]);
#pragma unroll
    for (int j = 0; j < 4; j++) acc[j] = mm(ah, bl[j], acc[j]);
#pragma unroll
    for (int j = 0; j < 4; j++) acc[j] = mm(al, bh[j], acc[j]);
  }
}

// k loop with the next stage's LDS-DMA spread over the MFMAs: the wave's 8
// pieces (4 of A, 4 of B) are issued two per row block over the first four of
// its eight row blocks, between the MFMAs,
// instead of as one block of address arithmetic + m0 writes at the top of the
// iteration (where both waves of a SIMD issued them at once, right after the
// barrier, with no matrix work to hide behind).  Source pointers are computed
// once per tile; the loads of the last iteration re-read the last k block
// (clamped) so the body is straight-line.
// AUXA: cache policy of the A pieces (16: sc1, rows packed by other CUs
// while this kernel runs)
template <bool BFM, int AUXA = 0, bool TR = false>
__device__ __forceinline__ void p256_kloop_spread(const _Float16 *A, const _Float16 *B, int M, int N, int KB, int m0,
                                                  int n0, int kb0, int nk, unsigned char *lds, int wm, int wn, int fr,
                                                  int fq, floatx4 (&acc)[8][4]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const _Float16 *src[8];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const int q = w * 4 + (i & 3);
    const int r = q * 8 + (lane >> 3);
    const int c = (lane & 7) ^ (r & 7);
    const int gr = i < 4 ? min(m0 + r, M - 1) : min(n0 + r, N - 1);
    src[i] = (i < 4 ? A : B) + ((long)gr * KB + kb0) * 64 + c * 8;
  }
#pragma unroll
  for (int i = 0; i < 8; i++) {
    if (i < 4) __builtin_amdgcn_global_load_lds(src[i], lds + (w * 4 + i) * 1024, 16, 0, AUXA);
    else __builtin_amdgcn_global_load_lds(src[i], lds + TILEB2 + (w * 4 + (i & 3)) * 1024, 16, 0, 0);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int it = 0; it < nk; it++) {
    unsigned char *cur = lds + (it & 1) * 2 * TILEB2;
    unsigned char *nxt = lds + ((it + 1) & 1) * 2 * TILEB2;
    const long adv = (long)min(it + 1, nk - 1) * 64;
    halfx8 bh[4], bl[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      bh[j] = frag(cur + TILEB2, wn + j * 16 + fr, fq);
      bl[j] = frag(cur + TILEB2, wn + j * 16 + fr, 4 + fq);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
      if (i < 4) {  // two pieces per row block of the first half: the last lands behind half the MFMAs
#pragma unroll
        for (int h = 2 * i; h < 2 * i + 2; h++) {
          if (h < 4) __builtin_amdgcn_global_load_lds(src[h] + adv, nxt + (w * 4 + h) * 1024, 16, 0, AUXA);
          else __builtin_amdgcn_global_load_lds(src[h] + adv, nxt + TILEB2 + (w * 4 + (h & 3)) * 1024, 16, 0, 0);
        }
      }
      const halfx8 ah = frag(cur, wm + i * 16 + fr, fq);
      const halfx8 al = frag(cur, wm + i * 16 + fr, 4 + fq);
      p256_row<BFM, TR>(acc[i], ah, al, bh, bl);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
}

}  // namespace
}  // namespace kctc
