// x3p_pack.hip -- the pack passes of the packed GEMM (gemm_x3p.h): fp32 rows
// or columns (the transpose) -> [rows][KB][64] split-fp16 with a per-row
// exponent (x3p_pack_rows / _cols) or bf16 (bf16_pack_rows / _cols), run once
// per operand.  The layouts are described in x3p_common.h.
#include "x3p_common.h"

namespace kctc {
namespace {

// Row packing: one wave per row; lane l holds k = 4 l + 256 i (i < KW), so a
// row of up to 256 KW values is read once.  bound > 0: fixed exponent.
template <int KW>
__global__ __launch_bounds__(256) void pack_rows_kernel(const float *__restrict__ X, long ldx, int R, int K, int KB,
                                                        long sX, _Float16 *__restrict__ out, long sOut,
                                                        int *__restrict__ eout, long sE, float bound, int vec) {
  const int b = blockIdx.y;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= R) return;
  const float *x = X + (long)b * sX + (long)r * ldx;
  floatx4 v[KW];
  float mx = 0.f;
#pragma unroll
  for (int i = 0; i < KW; i++) {
    const int k = 4 * lane + 256 * i;
    floatx4 t = {0.f, 0.f, 0.f, 0.f};
    if (vec && k + 3 < K) {
      t = *reinterpret_cast<const floatx4 *>(x + k);
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++) t[j] = k + j < K ? x[k + j] : 0.f;
    }
    v[i] = t;
    mx = fmaxf(mx, fmaxf(fmaxf(fabsf(t[0]), fabsf(t[1])), fmaxf(fabsf(t[2]), fabsf(t[3]))));
  }
  int e;
  if (bound > 0.f) {
    e = split_exp_d(bound);
  } else {
    mx = wave_max_l63(mx);
    e = split_exp_d(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(mx), 63)));
  }
  _Float16 *o = out + (long)b * sOut + (long)r * KB * 64;
#pragma unroll
  for (int i = 0; i < KW; i++) {
    const int k = 4 * lane + 256 * i;
    if (k < KB * 32) {
      halfx4 h, l;
      split4(v[i], e, h, l);
      const int kb = k >> 5, off = k & 31;
      *reinterpret_cast<halfx4 *>(o + kb * 64 + off) = h;
      *reinterpret_cast<halfx4 *>(o + kb * 64 + 32 + off) = l;
    }
  }
  if (lane == 0 && eout) eout[(long)b * sE + r] = e;
}

// one item: 64 columns x KPI consecutive 32-k blocks (KPI = 4, 512
// contiguous bytes per packed row, measured slower: configs[1] dGates^T
// 351 -> 511 us, fewer blocks in flight)
constexpr int KPI = 1;
__device__ __forceinline__ void pack_cols_item(const float *__restrict__ X, long ldx, int R, int Cn, int KB, int shift,
                                               long sX, _Float16 *__restrict__ out, long sOut, int *__restrict__ eout,
                                               long sE, const unsigned *__restrict__ cmax, long sCm, float bound,
                                               int bx, int kq, int b, float (*tile)[65]) {
  const int c0 = bx * 64, kb0 = kq * KPI;
  const float *x = X + (long)b * sX;
  const int t = threadIdx.x;
  // load KPI * 32 rows x 64 columns (each row: 64 consecutive floats), 16 B
  // per lane where the rows are 16-B aligned (4 rows per wave instruction)
  if (((reinterpret_cast<unsigned long>(x) & 15) | (ldx & 3)) == 0) {
#pragma unroll
    for (int i = 0; i < 2 * KPI; i++) {
      const int kr = (t >> 4) + 16 * i, cc = (t & 15) * 4;
      const int k = kb0 * 32 + kr, src = k - shift;
      floatx4 v = {0.f, 0.f, 0.f, 0.f};
      if (k < R && src >= 0 && src < R) {
        const float *xr = x + (long)src * ldx + c0 + cc;
        if (c0 + cc + 3 < Cn) {
          v = *reinterpret_cast<const floatx4 *>(xr);
        } else {
#pragma unroll
          for (int e = 0; e < 4; e++) v[e] = c0 + cc + e < Cn ? xr[e] : 0.f;
        }
      }
#pragma unroll
      for (int e = 0; e < 4; e++) tile[kr][cc + e] = v[e];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8 * KPI; i++) {
      const int kr = (t >> 6) + 4 * i, cc = t & 63;
      const int k = kb0 * 32 + kr, src = k - shift;
      float v = 0.f;
      if (k < R && src >= 0 && src < R && c0 + cc < Cn) v = x[(long)src * ldx + c0 + cc];
      tile[kr][cc] = v;
    }
  }
  __syncthreads();
  const int c = t >> 2, part = t & 3;
  if (c0 + c < Cn) {
    const int e = bound > 0.f ? split_exp_d(bound)
                              : split_exp_d(__uint_as_float(cmax[(long)b * sCm + c0 + c]));
    _Float16 *o = out + (long)b * sOut + ((long)(c0 + c) * KB + kb0) * 64;
#pragma unroll
    for (int q = 0; q < KPI; q++) {
      if (kb0 + q >= KB) break;
      halfx8 h, l;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const float xv = ldexpf(tile[q * 32 + part * 8 + j][c], e);
        h[j] = (_Float16)xv;
        l[j] = (_Float16)(xv - (float)h[j]);
      }
      *reinterpret_cast<halfx8 *>(o + q * 64 + part * 8) = h;
      *reinterpret_cast<halfx8 *>(o + q * 64 + 32 + part * 8) = l;
    }
    if (kb0 == 0 && part == 0 && eout) eout[(long)b * sE + c0 + c] = e;
  }
}

// Column packing (transpose): packed row c = column c of X, K = X's rows
// (k -> X row k - shift, zero outside [0, R)).  Exponent from cmax[c] (max |x|
// of the column, float bits) or the bound.  Item: 64 columns x KPI 32-k blocks
// (grid (columns / 64, KB / KPI, batch)).  With `avoid` (beside a pinned
// recurrence, X3PArgs::avoid_word) a 1-D grid takes runs of 8 items from
// a zeroed counter and the blocks on the recurrence's XCDs leave at once: a
// stream of short blocks cycling through its CUs kept the recurrence's
// workgroups from becoming resident for the length of the pack (configs[1]:
// ~230 us a layer).
__global__ __launch_bounds__(256) void pack_cols_kernel(const float *__restrict__ X, long ldx, int R, int Cn, int KB,
                                                        int shift, long sX, _Float16 *__restrict__ out, long sOut,
                                                        int *__restrict__ eout, long sE,
                                                        const unsigned *__restrict__ cmax, long sCm, float bound,
                                                        const unsigned *avoid, int nxcd, int batch, int *counter) {
  __shared__ float tile[32 * KPI][65];
  __shared__ int bc;
  if (!avoid) {
    pack_cols_item(X, ldx, R, Cn, KB, shift, sX, out, sOut, eout, sE, cmax, sCm, bound, blockIdx.x, blockIdx.y,
                   blockIdx.z, tile);
    return;
  }
  if (avoid_here(avoid, nxcd, &bc)) return;
  const int gx = (Cn + 63) / 64, KQ = (KB + KPI - 1) / KPI;
  const int items = gx * KQ * batch;
  while (true) {
    __syncthreads();  // bc and the tile are reused
    if (threadIdx.x == 0) bc = atomicAdd(counter, 8);
    __syncthreads();
    const int i0 = __builtin_amdgcn_readfirstlane(bc);
    if (i0 >= items) break;
    for (int it = i0; it < min(items, i0 + 8); it++) {
      const int bx = it % gx, r = it / gx;
      pack_cols_item(X, ldx, R, Cn, KB, shift, sX, out, sOut, eout, sE, cmax, sCm, bound, bx, r % KQ, r / KQ, tile);
      __syncthreads();
    }
  }
}

// bf16 packing: out[b][r][kb][64] = bf16(x[r][64 kb + j]), zero past K.
// Rows: one wave per row, lane l holds k = 4 l + 256 i.
template <int KW>
__global__ __launch_bounds__(256) void bf16_pack_rows_kernel(const float *__restrict__ X, long ldx, int R, int K,
                                                             int KB, long sX, __bf16 *__restrict__ out, long sOut,
                                                             int vec) {
  const int b = blockIdx.y;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= R) return;
  const float *x = X + (long)b * sX + (long)r * ldx;
  __bf16 *o = out + (long)b * sOut + (long)r * KB * 64;
#pragma unroll
  for (int i = 0; i < KW; i++) {
    const int k = 4 * lane + 256 * i;
    if (k >= KB * 64) continue;
    floatx4 t = {0.f, 0.f, 0.f, 0.f};
    if (vec && k + 3 < K) {
      t = *reinterpret_cast<const floatx4 *>(x + k);
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++) t[j] = k + j < K ? x[k + j] : 0.f;
    }
    bf16x4 h;
#pragma unroll
    for (int j = 0; j < 4; j++) h[j] = (__bf16)t[j];
    *reinterpret_cast<bf16x4 *>(o + k) = h;
  }
}
// Columns (transpose): packed row c = column c of X over its R rows (row
// k - shift, zero outside).  Block: 64 columns x one 64-k block.
__global__ __launch_bounds__(256) void bf16_pack_cols_kernel(const float *__restrict__ X, long ldx, int R, int Cn,
                                                             int KB, int shift, long sX, __bf16 *__restrict__ out,
                                                             long sOut) {
  __shared__ float tile[64][65];
  const int b = blockIdx.z, c0 = blockIdx.x * 64, kb = blockIdx.y;
  const float *x = X + (long)b * sX;
  const int t = threadIdx.x;
  if (((reinterpret_cast<unsigned long>(x) & 15) | (ldx & 3)) == 0) {  // 16 B per lane (as pack_cols_item)
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int kr = (t >> 4) + 16 * i, cc = (t & 15) * 4;
      const int src = kb * 64 + kr - shift;
      floatx4 v = {0.f, 0.f, 0.f, 0.f};
      if (kb * 64 + kr < R && src >= 0 && src < R) {
        const float *xr = x + (long)src * ldx + c0 + cc;
        if (c0 + cc + 3 < Cn) {
          v = *reinterpret_cast<const floatx4 *>(xr);
        } else {
#pragma unroll
          for (int e = 0; e < 4; e++) v[e] = c0 + cc + e < Cn ? xr[e] : 0.f;
        }
      }
#pragma unroll
      for (int e = 0; e < 4; e++) tile[kr][cc + e] = v[e];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const int kr = (t >> 6) + 4 * i, cc = t & 63;
      const int src = kb * 64 + kr - shift;
      float v = 0.f;
      if (kb * 64 + kr < R && src >= 0 && src < R && c0 + cc < Cn) v = x[(long)src * ldx + c0 + cc];
      tile[kr][cc] = v;
    }
  }
  __syncthreads();
  const int c = t >> 2, part = t & 3;
  if (c0 + c >= Cn) return;
  __bf16 *o = out + (long)b * sOut + ((long)(c0 + c) * KB + kb) * 64 + part * 16;
  bf16x8 h0, h1;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    h0[j] = (__bf16)tile[part * 16 + j][c];
    h1[j] = (__bf16)tile[part * 16 + 8 + j][c];
  }
  *reinterpret_cast<bf16x8 *>(o) = h0;
  *reinterpret_cast<bf16x8 *>(o + 8) = h1;
}

}  // namespace

void bf16_pack_rows(hipStream_t s, const float *X, long ldx, int R, int K, __bf16 *out, int batch, long sX,
                    long sOut) {
  if (R <= 0 || K <= 0 || batch <= 0) return;
  const int KB = (K + 63) / 64;
  const int vec = ((uintptr_t)X % 16 == 0) && (ldx % 4 == 0) && (sX % 4 == 0);
  const dim3 grid(ceil_div(R, 4), batch);
  const bool ok = x3p_with_kw(KB * 64, [&](auto kw) {
    hipLaunchKernelGGL(bf16_pack_rows_kernel<decltype(kw)::value>, grid, dim3(256), 0, s, X, ldx, R, K, KB, sX, out,
                       sOut, vec);
  });
  if (!ok) throw std::invalid_argument("bf16_pack_rows: K > 4096");
}

void bf16_pack_cols(hipStream_t s, const float *X, long ldx, int R, int Cn, int shift, __bf16 *out) {
  if (R <= 0 || Cn <= 0) return;
  const int KB = (R + 63) / 64;
  hipLaunchKernelGGL(bf16_pack_cols_kernel, dim3(ceil_div(Cn, 64), KB, 1), dim3(256), 0, s, X, ldx, R, Cn, KB, shift,
                     0L, out, 0L);
}

void x3p_pack_rows(hipStream_t s, const float *X, long ldx, int R, int K, _Float16 *out, int *eout, float bound,
                   int batch, long sX, long sOut, long sE) {
  if (R <= 0 || K <= 0 || batch <= 0) return;
  const int KB = (K + 31) / 32;
  const int vec = ((uintptr_t)X % 16 == 0) && (ldx % 4 == 0) && (sX % 4 == 0);
  const dim3 grid(ceil_div(R, 4), batch);
  // lanes cover KW*256 values of a row; the packed row also needs the zero pad up to KB*32
  const bool ok = x3p_with_kw(KB * 32, [&](auto kw) {
    hipLaunchKernelGGL(pack_rows_kernel<decltype(kw)::value>, grid, dim3(256), 0, s, X, ldx, R, K, KB, sX, out, sOut,
                       eout, sE, bound, vec);
  });
  if (!ok) throw std::invalid_argument("x3p_pack_rows: K > 4096");
}

void x3p_pack_cols(hipStream_t s, const float *X, long ldx, int R, int Cn, int shift, _Float16 *out, int *eout,
                   const unsigned *cmax, float bound, PackAvoid avoid) {
  if (R <= 0 || Cn <= 0) return;
  const int KB = (R + 31) / 32;
  const long z = 0;  // one matrix: no batch strides
  if (avoid.word) {
    const long items = (long)ceil_div(Cn, 64) * ceil_div(KB, KPI);
    if (!avoid.counter || items + 8 >= (1L << 31)) throw std::invalid_argument("x3p_pack_cols: avoid needs a counter");
    hipLaunchKernelGGL(pack_cols_kernel, dim3((int)std::min<long>((items + 7) / 8, 1024)), dim3(256), 0, s, X, ldx, R,
                       Cn, KB, shift, z, out, z, eout, z, cmax, z, bound, avoid.word, avoid.nxcd, 1, avoid.counter);
    return;
  }
  hipLaunchKernelGGL(pack_cols_kernel, dim3(ceil_div(Cn, 64), ceil_div(KB, KPI), 1), dim3(256), 0, s, X, ldx, R, Cn, KB,
                     shift, z, out, z, eout, z, cmax, z, bound, nullptr, 0, 1, nullptr);
}

}  // namespace kctc
