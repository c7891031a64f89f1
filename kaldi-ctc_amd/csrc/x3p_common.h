// x3p_common.h -- private to the packed-GEMM units (x3p_gemm.hip,
// x3p_stream.hip, x3p_pack.hip): the kernel-argument struct, the tile
// constants and LDS image, the waits on other workgroups, the job helpers and
// the launch helpers they share.  Everything sits in an anonymous namespace:
// each unit gets its own copy and a kernel is defined in exactly one of them.
//
// The fp32-class product of gemm.hip's x3 kernel, with the fp32 -> (hi, lo)
// conversion moved out of the GEMM's staging path into pack passes that run
// once per operand:
//
//   packed operand P[r][kb][64] (fp16): the 32 values k = 32 kb .. 32 kb + 31
//   of row r, scaled by 2^e[r], as 32 hi halves then 32 lo halves (128 B);
//   e[r] puts the row's max |x| in [2^13, 2^14) (or comes from a bound on |x|).
//
// C[m][n] = alpha * 2^-(eA[m] + eB[n]) * sum_k (Ahi Bhi + Ahi Blo + Alo Bhi)
//           (+ beta C + bias), both operands packed along K.
//
// The LDS image of a tile is rows x 128 B with the eight 16-B chunks of row r
// stored at chunk (c ^ (r & 7)) -- the swizzle is applied to the per-lane
// SOURCE address, so the DMA destination (global_load_lds_dwordx4, 16 B per
// lane) stays lane-linear -- and the fragment reads (ds_read_b128, rows
// fr = lane & 15, chunk fq or 4 + fq) are conflict-free.
#pragma once
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "gemm_x3p.h"

namespace kctc {
namespace {

constexpr int TB = 128;          // tile rows (M) = tile cols (N)
constexpr int NTH = 256;
constexpr int ROWB = 128;        // bytes per packed row block (64 halves)
constexpr int TILEB = TB * ROWB; // 16 KB per operand tile per stage
constexpr int TB2 = 256, NTH2 = 512, TILEB2 = TB2 * ROWB;  // the 256 tile (x3p_tile256.h): 32 KB per operand tile per stage
// dynamic LDS of a launch: [2 stages][A tile | B tile] and the job words; streaming launches
// of the 128 tile ask for 96 KB so that no block shares a CU with a producer workgroup
constexpr size_t kLdsBase = 2 * 2 * TILEB + 16, kLdsStream = 96 * 1024;
constexpr size_t kLds256 = 2 * 2 * (size_t)TILEB2 + 16;
constexpr unsigned long long kWaitTicks = 300000000ull;  // streaming waits: 3 s of the 100 MHz clock
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));
typedef _Float16 halfx4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct PParams {
  const _Float16 *A, *B;
  const int *eA, *eB;
  float *C;
  const float *bias, *bias2;
  long ldc;
  long sA, sB, sC, sBias, seA, seB;  // batch strides (A, B in halves; eA, eB in ints)
  int M, N, KB;
  int gx, tiles, batch, split, kbchunk;
  float alpha, beta;
  float *ws;
  int *counter;
  int eA0, eB0;
  const unsigned *sflags;  // streaming mode: producer flag lines
  int snwg, sT, sN;
  int srg;                 // producer row groups (flag lines and images per group)
  int sgsh;                // log2 of the sequences per row group (4: 16, 3: 8)
  int nrt;                 // row tiles
  long sxs;                // halves per producer step image
  long sxg;                // halves per row group's part of a step image
  int sdir;                // streaming: K split by producer direction (two half-K jobs per C tile, see fwd_combine)
  unsigned *serr;          // producer's error word (wait timeout)
  const unsigned *xcd_word;  // XCDs of a pinned producer (X3PBwdStream::xcd_word), xcd_count of them
  int xcd_count;
  // backward stream (x3p_bwd_stream_kernel)
  const float *E;          // source rows of direction d: E + row * lde + d * edoff (KB * 32 floats)
  long lde, edoff;
  int P;                   // pack jobs per row tile
  int *done;               // [2][nrt] pack jobs finished
  int *arrive;             // [nrt][gx] direction partials arrived (+1) / partial published (+2)
  float *part;             // [M][N] the first direction's partial
  const unsigned *avoid;   // X3PArgs::avoid_word, avoid_xcds
  int nxcd;
  // row stream (x3p_bwd_stream256_kernel) off a FORWARD producer: direction 0
  // frames ascending, direction 1 descending; bias + bias2 of column c at
  // (c / bcols) * sBias + c % bcols, added by the second partial
  int fwdp, bcols;
  // split-K tail: the last tailr row-tile slots of each direction (ready only
  // at the producer's last steps) run as tails K-splits each; their tiles'
  // partials meet in part2 ([tail tile][tails + 1][256 x 256])
  int tailr, tails;
  float *part2;
};

// LDS-DMA of one k block of 32 rows per wave into the swizzled tile image: the
// 128 rows of the 128 tile with 4 waves, the 256 rows of the 256 tile with 8
template <int AUX = 0>
__device__ __forceinline__ void issue_tile(const _Float16 *__restrict__ P, int rows, int r0, int KB, int kb,
                                           unsigned char *dst) {
  // wave w fills rows [32 w, 32 w + 32) of the tile: 4 instructions of 8 rows x 128 B
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int q = w * 4 + i;
    const int r = q * 8 + (lane >> 3);
    const int c = (lane & 7) ^ (r & 7);
    int gr = r0 + r;
    gr = gr < rows ? gr : rows - 1;  // rows past the edge: any valid row (results discarded)
    const _Float16 *src = P + ((long)gr * KB + kb) * 64 + c * 8;
    __builtin_amdgcn_global_load_lds(src, dst + q * 1024, 16, 0, AUX);
  }
}

__device__ __forceinline__ halfx8 frag(const unsigned char *tile, int row, int chunk) {
  return *reinterpret_cast<const halfx8 *>(tile + row * ROWB + ((chunk ^ (row & 7)) << 4));
}

// ---- waits on other workgroups ------------------------------------------
// All polling is done by wave 0 with every lane active and every exit
// decision made wave-uniform (readfirstlane), and the waves choose between
// polling and waiting on the barrier by a scalar branch on their wave index.
// (Thread-0 spin loops followed by a barrier let the compiler structure the
// barrier into exec-masked control flow: waves 1-3 then ran on without wave
// 0, observed as a hang on the GPU.)
__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }

__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, o));
  return __builtin_amdgcn_readfirstlane(v);
}

// wave-level: true once every flag word f[32 g], g < nwg, holds >= need
// (false after a timeout or another party's error; then err bit 2 is set)
__device__ __forceinline__ unsigned wave_flags_min(const unsigned *f, int nwg) {
  unsigned m = 0xffffffffu;
  for (int g = threadIdx.x & 63; g < nwg; g += 64)
    m = min(m, __hip_atomic_load(f + 32L * g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  return wave_min_u32(m);
}
// A wait that runs out of time itself (no error posted yet) also sets bit
// 8 + site of err: which wait it was (0 producer rows, 1 pack jobs / tile
// arrivals, 2 pinned-XCD registrations, 3 producer epochs) -- the other
// bits are set by whoever saw the error first.
__device__ __forceinline__ bool wave_timed_out(unsigned *err, int spins, unsigned long long t0, int site) {
  if ((spins & 255) != 255) return false;
  const unsigned e = err ? __builtin_amdgcn_readfirstlane(__hip_atomic_load(err, __ATOMIC_RELAXED,
                                                                            __HIP_MEMORY_SCOPE_AGENT)) : 0u;
  if (e != 0u) return true;
  const bool late = __builtin_amdgcn_s_memrealtime() - t0 > kWaitTicks;
  if (late && err && (threadIdx.x & 63) == 0) atomicOr(err, 0x100u << site);
  return late;
}
__device__ __forceinline__ void wave_fail(unsigned *err) {
  if ((threadIdx.x & 63) == 0 && err) atomicOr(err, 2u);
}

// Waiting for a producer that is `gap` steps (~3 us each) short: sleep for
// gap - 1 steps instead of re-polling its flag lines every ~0.2 us -- up to
// 176 blocks poll the same lines the recurrence itself polls and stores
__device__ __forceinline__ void backoff(int gap) {
  if (gap > 2) {
    const int n = min(gap - 1, 64);
    for (int i = 0; i < n; i++) __builtin_amdgcn_s_sleep(80);  // 80 x 64 clocks: ~2.4 us at 2.1 GHz
  } else {
    __builtin_amdgcn_s_sleep(8);
  }
}

// wave 0 waits for a device counter to reach v, then the workgroup barrier
__device__ __forceinline__ void wait_count(const int *a, int v, unsigned *err) {
  if (wave_id() == 0) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    bool failed = false;
    int i = 0;
    while (true) {
      const int x = __builtin_amdgcn_readfirstlane(__hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      if (x >= v) break;
      failed = wave_timed_out(err, i++, t0, 1);
      if (failed) break;
      __builtin_amdgcn_s_sleep(4);
    }
    if (failed) wave_fail(err);
  }
  __syncthreads();
}

// true when this block runs on an XCD that an XCD-pinned producer occupies
// (block-uniform): wave 0 waits until the producer's workgroups registered
// p.xcd_count XCDs in *p.xcd_word (bounded, as the other waits), then looks
// up its own.  Such blocks leave before taking work -- spinning on the
// producer's flags there they would keep its workgroups off their CUs.
__device__ bool on_pinned_xcd(const PParams &p, int *bc) {
  if (!p.xcd_word) return false;
  if (wave_id() == 0) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    unsigned m = 0;
    bool failed = false;
    int i = 0;
    while (true) {
      m = __builtin_amdgcn_readfirstlane(__hip_atomic_load(p.xcd_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      if (__builtin_popcount(m) >= p.xcd_count) break;
      failed = wave_timed_out(p.serr, i++, t0, 2);
      if (failed) break;
      __builtin_amdgcn_s_sleep(4);
    }
    unsigned x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
    if (threadIdx.x == 0) *bc = failed ? 1 : (int)((m >> (x & 0xfu)) & 1u);
    if (failed) wave_fail(p.serr);
  }
  __syncthreads();
  return __builtin_amdgcn_readfirstlane(*bc) != 0;
}

// wait until every workgroup of producer direction d has published epoch
// >= need (seen[d]: the last minimum seen, LDS)
__device__ void wait_epoch(const PParams &p, int d, int need, int *seen) {
  const bool ok = __builtin_amdgcn_readfirstlane(seen[d] >= need);
  __syncthreads();
  if (ok) return;
  if (wave_id() == 0) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    bool failed = false;
    int m = 0, spins = 0;
    while (true) {
      m = 1 << 30;
      for (int gi = 0; gi < p.srg; gi++)
        m = min(m, (int)wave_flags_min(p.sflags + 32L * (2 * gi + d) * p.snwg, p.snwg));
      if (m >= need) break;
      failed = wave_timed_out(p.serr, spins++, t0, 3);
      if (failed) break;
      backoff(need - m);
    }
    if (threadIdx.x == 0) seen[d] = failed ? 1 << 30 : m;
    if (failed) wave_fail(p.serr);
  }
  __syncthreads();
}

__device__ __forceinline__ void decode_tile(const PParams &p, int id, int total, bool remap, int &tm, int &tn,
                                            int &b, int &ks) {
  const int q = total >> 3, rr = total & 7, xcd = id & 7, loc = id >> 3;
  const int wl = remap ? (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + loc : id;
  const int bz = wl / p.tiles, wg = wl - bz * p.tiles;
  if (remap) {
    // groups of 8 tile rows, column by column inside a group: the 32 blocks
    // an XCD runs at once cover 8 row x 4 column tiles (12 panels of A and B
    // in its L2) instead of one row of tiles (1 + gx panels); 8192^3 bf16
    // 0.42 -> 0.45 of peak, the train step's shapes unchanged (±1 %)
    const int rows = p.tiles / p.gx, per = 8 * p.gx;
    const int grp = wg / per, first = grp * 8, w = wg - grp * per;
    const int gsz = min(8, rows - first);
    tm = first + w % gsz; tn = w / gsz;
  } else {
    tn = wg % p.gx; tm = wg / p.gx;
  }
  b = bz % p.batch; ks = bz / p.batch;
}

// the next job of a persistent block: thread 0 takes an id from the counter,
// every thread gets it (slot: an LDS word).  The second barrier keeps the
// slot from being rewritten while a wave still reads it.
__device__ __forceinline__ int next_job(int *counter, int *slot) {
  if (threadIdx.x == 0) *slot = atomicAdd(counter, 1);
  __syncthreads();
  const int id = __builtin_amdgcn_readfirstlane(*slot);
  __syncthreads();
  return id;
}

// beside a pinned recurrence (X3PArgs::avoid_word): true on one of its XCDs
// (block-uniform; the word only ever gains bits)
__device__ __forceinline__ bool avoid_here(const unsigned *avoid, int nxcd, int *bc) {
  if (!avoid) return false;
  if (threadIdx.x == 0) {
    unsigned x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
    const unsigned m = __hip_atomic_load(avoid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *bc = (int)((m >> (x & 0xfu)) & 1u) && __builtin_popcount(m) < nxcd;
  }
  __syncthreads();
  return __builtin_amdgcn_readfirstlane(*bc) != 0;
}

__device__ __forceinline__ int split_exp_d(float mx) {
  int e = 0;
  (void)frexpf(mx, &e);
  return 14 - e;
}

__device__ __forceinline__ void split4(floatx4 v, int e, halfx4 &h, halfx4 &l) {
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const float x = ldexpf(v[j], e);
    h[j] = (_Float16)x;
    l[j] = (_Float16)(x - (float)h[j]);
  }
}

// ---- host side ------------------------------------------------------------
// Launch with dynamic LDS: the kernel's limit (above the 64 KB default) is
// raised once per process, at its first launch.
template <auto Kern, typename... Args>
void x3p_launch(dim3 grid, int threads, size_t lds, hipStream_t s, const Args &...args) {
  static const bool attr = [lds] {
    KCTC_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds));
    return true;
  }();
  (void)attr;
  hipLaunchKernelGGL(Kern, grid, dim3(threads), lds, s, args...);
}

// Row passes hold a row in registers, lane l the values k = 4 l + 256 i,
// i < KW: calls f(integral_constant<int, KW>) with the smallest KW of KW0, 2 KW0,
// .. 16 that covers `need` values; false when a row is longer than 4096.
template <int KW0 = 1, typename F>
bool x3p_with_kw(int need, F &&f) {
  if (need <= 256 * KW0) {
    f(std::integral_constant<int, KW0>{});
    return true;
  }
  if constexpr (KW0 < 16) return x3p_with_kw<2 * KW0>(need, f);
  return false;
}

// The kernel arguments every launch fills the same way: the problem, its tile
// grid on tb x tb tiles, and the producer a streaming launch follows.
struct X3PProducer {
  const unsigned *flags;
  int nwg, T, N, rg;
  unsigned *err;
  const unsigned *xcd_word;
  int xcd_count;
};
inline PParams x3p_problem(int M, int N, int KB, int tb, const _Float16 *A, const int *eA, const _Float16 *B,
                           const int *eB, float *C, long ldc, const float *bias, const float *bias2, long sBias,
                           int *counter, const X3PProducer &pr) {
  PParams p{};
  p.M = M; p.N = N; p.KB = KB;
  p.A = A; p.eA = eA; p.B = B; p.eB = eB; p.C = C; p.ldc = ldc;
  p.bias = bias; p.bias2 = bias2; p.sBias = sBias;
  p.gx = ceil_div(N, tb); p.nrt = ceil_div(M, tb); p.tiles = p.gx * p.nrt;
  p.counter = counter;
  p.sflags = pr.flags; p.snwg = pr.nwg; p.sT = pr.T; p.sN = pr.N; p.srg = pr.rg; p.serr = pr.err;
  p.xcd_word = pr.xcd_word; p.xcd_count = pr.xcd_count;
  return p;
}

}  // namespace
}  // namespace kctc
