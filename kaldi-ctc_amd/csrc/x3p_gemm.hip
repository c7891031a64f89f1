// x3p_gemm.hip -- the tile GEMMs on packed operands (gfx950): gemm_x3p and
// gemm_x3p_pair (gemm_x3p.h).  Three kernels: the 128-tile GEMM with its
// forward image-stream mode (tile: x3p_tile128.h), the 256-tile GEMM and its
// pair launch for the large shapes (k loop: x3p_tile256.h), and the split-K
// reduction.  Packing is x3p_pack.hip, the row streams are x3p_stream.hip.
#include "x3p_tile128.h"
#include "x3p_tile256.h"

namespace kctc {
namespace {

// Row tile of the i-th work slot in readiness order of a bidirectional
// producer: tile rt (frames t0..t1) is complete once direction 0 has reached
// t1 and direction 1 has reached T-1-t0, i.e. at step max(t1, T-1-t0): the
// middle of the sequence first, then alternately outwards.
__device__ __forceinline__ int stream_row_tile(int i, int nrt, int sT, int sN) {
  // ready step of tile rt: max(t1(rt), T-1-t0(rt)); sort key, ties by rt.
  // Binary-search-free: walk outwards from the middle tile.
  const int tmid = (sT - 1) / 2;
  const int mid = min(nrt - 1, (tmid * sN) / TB);
  // interleave mid, mid-1, mid+1, mid-2, ... (exact ordering of ready steps
  // is not required for correctness, only for overlap)
  const int L = mid, R = nrt - 1 - mid;  // tiles left / right of the middle one
  if (i > 2 * min(L, R)) return L < R ? mid + (i - L) : mid - (i - R);
  const int k = (i + 1) / 2;
  return (i & 1) ? mid - k : mid + k;
}

__host__ __device__ inline int stream_total(const PParams &p) { return p.nrt * p.batch * p.gx * (p.sdir ? 2 : 1); }

template <bool STREAM, bool BFM = false>
__global__ __launch_bounds__(NTH, 2) void gemm_x3p_kernel(PParams p) {
  // ONE shared array (a second __shared__ object can make hipcc wait vmcnt(0)
  // before LDS reads while a DMA is in flight); streaming launches ask for
  // 96 KB so that no block shares a CU with a producer workgroup
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  int *next = reinterpret_cast<int *>(lds + 2 * 2 * TILEB);
  int *prog = next + 1;
  const int total = STREAM ? stream_total(p) : p.tiles * p.batch * p.split;
  if (STREAM && threadIdx.x == 0) { prog[0] = -1; prog[1] = -1; }
  if (STREAM && on_pinned_xcd(p, prog + 2)) return;  // before taking any job
  if (p.counter) {
    while (true) {
      const int id = next_job(p.counter, next);
      if (id >= total) break;
      int tm, tn, b, ks;
      if (STREAM) {  // id = (row slot * batch + b) * gx + tn; no split-K
        tn = id % p.gx;
        const int rest = id / p.gx;
        b = rest % p.batch;
        const int slot = rest / p.batch;
        if (p.sdir) {  // slot = 2 j + producer direction: its K half of row tile j (dir 0) / nrt-1-j (dir 1)
          const int pd = slot & 1, j = slot >> 1;
          x3p_tile<1, BFM>(p, lds, pd == 0 ? j : p.nrt - 1 - j, tn, b, pd, prog);
        } else {
          tm = stream_row_tile(slot, p.nrt, p.sT, p.sN);
          x3p_tile<1, BFM>(p, lds, tm, tn, b, 0, prog);
        }
      } else {
        decode_tile(p, id, total, false, tm, tn, b, ks);
        x3p_tile<0, BFM>(p, lds, tm, tn, b, ks, prog);
      }
    }
    return;
  }
  if (!STREAM) {
    for (int id = blockIdx.x; id < total; id += gridDim.x) {
      int tm, tn, b, ks;
      decode_tile(p, id, total, true, tm, tn, b, ks);
      x3p_tile<0, BFM>(p, lds, tm, tn, b, ks, prog);
    }
  }
}

template <bool BFM>
__device__ __forceinline__ void p256_tile(const PParams &p, unsigned char *lds, int tm, int tn, int b, int ks) {
  const _Float16 *A = p.A + (long)b * p.sA;
  const _Float16 *B = p.B + (long)b * p.sB;
  const int m0 = tm * TB2, n0 = tn * TB2;
  const int kb0 = ks * p.kbchunk, kb1 = min(p.KB, kb0 + p.kbchunk);
  const int nk = kb1 > kb0 ? kb1 - kb0 : 0;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wm = (wid >> 2) * 128, wn = (wid & 3) * 64;
  const int fr = lane & 15, fq = lane >> 4;
  floatx4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
  // the spread loop for split-fp16 (measured +4..10 %: dW 0.476 ->
  // 0.50-0.52, 8192^3 0.527 -> 0.555 of the f16 issue rate), the block loop
  // for bf16 (equal or 1-3 % faster there: fewer MFMAs per stage to hide the
  // DMA issue behind)
  if constexpr (!BFM) {
    if (nk > 0) p256_kloop_spread<BFM, 0, true>(A, B, p.M, p.N, p.KB, m0, n0, kb0, nk, lds, wm, wn, fr, fq, acc);
  } else {
    if (nk > 0) {
      issue_tile(A, p.M, m0, p.KB, kb0, lds);
      issue_tile(B, p.N, n0, p.KB, kb0, lds + TILEB2);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int it = 0; it < nk; it++) {
      unsigned char *cur = lds + (it & 1) * 2 * TILEB2;
      unsigned char *nxt = lds + ((it + 1) & 1) * 2 * TILEB2;
      if (it + 1 < nk) {
        issue_tile(A, p.M, m0, p.KB, kb0 + it + 1, nxt);
        issue_tile(B, p.N, n0, p.KB, kb0 + it + 1, nxt + TILEB2);
      }
      halfx8 bh[4], bl[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        bh[j] = frag(cur + TILEB2, wn + j * 16 + fr, fq);
        bl[j] = frag(cur + TILEB2, wn + j * 16 + fr, 4 + fq);
      }
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const halfx8 ah = frag(cur, wm + i * 16 + fr, fq);
        const halfx8 al = frag(cur, wm + i * 16 + fr, 4 + fq);
        p256_row<BFM, true>(acc[i], ah, al, bh, bl);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
  }
  // epilogue, transposed accumulators: acc[i][j][c] -> C[m0+wm+16i+fr][n0+wn+16j+4fq+c],
  // times 2^-(eA + eB); one 16-B store per (i, j) where the row piece is aligned
  const int *eA = p.eA ? p.eA + (long)b * p.seA : nullptr;
  const int *eB = p.eB ? p.eB + (long)b * p.seB : nullptr;
  float *W = p.split > 1 ? p.ws + ((long)ks * p.batch + b) * (long)p.M * p.N : nullptr;
  float *C = p.C + (long)b * p.sC;
  const float *bias = p.bias ? p.bias + (long)b * p.sBias : nullptr;
  const float *bias2 = p.bias2 ? p.bias2 + (long)b * p.sBias : nullptr;
  float *const O = W ? W : C;
  const long ldo = W ? p.N : p.ldc;
  const bool vec = ((reinterpret_cast<unsigned long>(O) & 15) == 0) && (ldo & 3) == 0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int col0 = n0 + wn + j * 16 + fq * 4;
    int eb[4];
    float badd[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const int col = col0 + c;
      eb[c] = col < p.N ? (eB ? eB[col] : p.eB0) : 0;
      badd[c] = 0.f;
      if (!W && col < p.N) {
        if (bias) badd[c] += bias[col];
        if (bias2) badd[c] += bias2[col];
      }
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int row = m0 + wm + i * 16 + fr;
      if (row >= p.M || col0 >= p.N) continue;
      const int ea = eA ? eA[row] : p.eA0;
      float *o = O + (long)row * ldo + col0;
      floatx4 v;
#pragma unroll
      for (int c = 0; c < 4; c++) {
        v[c] = ldexpf(acc[i][j][c], -(ea + eb[c]));
        if (!W) v[c] = p.alpha * v[c] + badd[c];
      }
      if (vec && col0 + 3 < p.N) {
        if (!W && p.beta != 0.f) {
          const floatx4 old = *reinterpret_cast<const floatx4 *>(o);
#pragma unroll
          for (int c = 0; c < 4; c++) v[c] += p.beta * old[c];
        }
        *reinterpret_cast<floatx4 *>(o) = v;
      } else {
#pragma unroll
        for (int c = 0; c < 4; c++) {
          if (col0 + c < p.N) {
            float x = v[c];
            if (!W && p.beta != 0.f) x += p.beta * o[c];
            o[c] = x;
          }
        }
      }
    }
  }
}

template <bool BFM>
__global__ __launch_bounds__(NTH2, 1) void gemm_p256_kernel(PParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];  // ONE shared array
  int *next = reinterpret_cast<int *>(lds + 2 * 2 * TILEB2);
  const int total = p.tiles * p.batch * p.split;
  if (avoid_here(p.avoid, p.nxcd, next + 1)) return;
  if (p.counter) {  // dynamic scheduling (beside a persistent kernel)
    while (true) {
      const int id = next_job(p.counter, next);
      if (id >= total) break;
      int tm, tn, b, ks;
      decode_tile(p, id, total, false, tm, tn, b, ks);
      p256_tile<BFM>(p, lds, tm, tn, b, ks);
    }
    return;
  }
  for (int id = blockIdx.x; id < total; id += gridDim.x) {
    int tm, tn, b, ks;
    decode_tile(p, id, total, true, tm, tn, b, ks);
    p256_tile<BFM>(p, lds, tm, tn, b, ks);
  }
}

// two problems, one job space (p's jobs, then q's), p's tile counter
template <bool BFM>
__global__ __launch_bounds__(NTH2, 1) void gemm_p256_pair_kernel(PParams p, PParams q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];  // ONE shared array
  int *next = reinterpret_cast<int *>(lds + 2 * 2 * TILEB2);
  const int t1 = p.tiles * p.batch * p.split, t2 = q.tiles * q.batch * q.split;
  if (avoid_here(p.avoid, p.nxcd, next + 1)) return;
  while (true) {
    const int id = next_job(p.counter, next);
    if (id >= t1 + t2) break;
    int tm, tn, b, ks;
    if (id < t1) {
      decode_tile(p, id, t1, false, tm, tn, b, ks);
      p256_tile<BFM>(p, lds, tm, tn, b, ks);
    } else {
      decode_tile(q, id - t1, t2, false, tm, tn, b, ks);
      p256_tile<BFM>(q, lds, tm, tn, b, ks);
    }
  }
}

__global__ __launch_bounds__(256) void x3p_splitk_reduce(PParams p) {
  const long total = (long)p.batch * p.M * p.N;
  const long MN = (long)p.M * p.N;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int b = (int)(e / MN);
    const long rem = e - (long)b * MN;
    const int row = (int)(rem / p.N), col = (int)(rem - (long)row * p.N);
    float s = 0.f;
    for (int k = 0; k < p.split; k++) s += p.ws[((long)k * p.batch + b) * MN + rem];
    float *c = p.C + (long)b * p.sC + (long)row * p.ldc + col;
    float v = p.alpha * s;
    if (p.bias) v += p.bias[(long)b * p.sBias + col];
    if (p.bias2) v += p.bias2[(long)b * p.sBias + col];
    if (p.beta != 0.f) v += p.beta * *c;
    *c = v;
  }
}

// uniform [-1, 1) halves (fp16 or bf16 bit patterns) from a counter hash
__global__ void fill_halves_kernel(unsigned short *p, long n, unsigned seed, int bf16) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    unsigned x = (unsigned)i * 2654435761u ^ seed;
    x ^= x >> 15; x *= 2246822519u; x ^= x >> 13; x *= 3266489917u; x ^= x >> 16;
    const float v = (float)(x >> 8) * (2.0f / 16777216.0f) - 1.0f;
    p[i] = bf16 ? __builtin_bit_cast(unsigned short, (__bf16)v) : __builtin_bit_cast(unsigned short, (_Float16)v);
  }
}
}  // namespace

float x3p_bench(hipStream_t s, int M, int N, int K, bool bf16, int iters, int split) {
  const int KB = bf16 ? (K + 63) / 64 : (K + 31) / 32;
  const long na = (long)M * KB * 64, nb = (long)N * KB * 64;
  _Float16 *A = nullptr, *B = nullptr;
  float *C = nullptr, *ws = nullptr;
  KCTC_HIP_CHECK(hipMalloc(&A, na * 2));
  KCTC_HIP_CHECK(hipMalloc(&B, nb * 2));
  KCTC_HIP_CHECK(hipMalloc(&C, (long)M * N * 4));
  if (split > 1) KCTC_HIP_CHECK(hipMalloc(&ws, (long)split * M * N * 4));
  hipLaunchKernelGGL(fill_halves_kernel, dim3(1024), dim3(256), 0, s, reinterpret_cast<unsigned short *>(A), na, 1u,
                     bf16 ? 1 : 0);
  hipLaunchKernelGGL(fill_halves_kernel, dim3(1024), dim3(256), 0, s, reinterpret_cast<unsigned short *>(B), nb, 2u,
                     bf16 ? 1 : 0);
  X3PArgs g;
  g.M = M; g.N = N; g.KB = KB; g.A = A; g.B = B; g.C = C; g.ldc = N; g.bf16 = bf16;
  g.split_k = split; g.ws = ws;
  for (int i = 0; i < 2; i++) gemm_x3p(s, g);
  hipEvent_t e0, e1;
  KCTC_HIP_CHECK(hipEventCreate(&e0));
  KCTC_HIP_CHECK(hipEventCreate(&e1));
  KCTC_HIP_CHECK(hipEventRecord(e0, s));
  for (int i = 0; i < iters; i++) gemm_x3p(s, g);
  KCTC_HIP_CHECK(hipEventRecord(e1, s));
  KCTC_HIP_CHECK(hipEventSynchronize(e1));
  float ms = 0.f;
  KCTC_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  (void)hipFree(A); (void)hipFree(B); (void)hipFree(C);
  if (ws) (void)hipFree(ws);
  return ms / iters;
}

bool x3p_use_256(int M, int N) { return M >= 192 && N >= 192; }

int x3p_pick_split(int M, int N, int KB, int batch) {
  const int tb = x3p_use_256(M, N) ? TB2 : TB;
  const long tiles = (long)ceil_div(M, tb) * ceil_div(N, tb) * batch;
  if (tiles >= 384 || KB < 16) return 1;
  long want = (512 + tiles - 1) / tiles;
  want = std::min<long>(want, KB / 8);
  want = std::min<long>(want, 32);
  return want < 1 ? 1 : (int)want;
}

// kernel parameters of a gemm_x3p call (t256: it runs on 256 x 256 tiles)
static PParams x3p_params(const X3PArgs &g, bool &t256) {
  t256 = !g.producer.lines && x3p_use_256(g.M, g.N);  // large shapes on 256 x 256 tiles
  PParams p = x3p_problem(g.M, g.N, g.KB, t256 ? TB2 : TB, g.A, g.eA, g.B, g.eB, g.C, g.ldc, g.bias, g.bias2, g.sBias,
                          g.tile_counter,
                          {g.producer.lines, g.producer.nwg, g.stream_T, g.stream_N, g.stream_rg, g.stream_err,
                           g.producer.xcd_word, g.producer.xcd_count});
  p.sA = g.sA; p.sB = g.sB; p.sC = g.sC; p.seA = g.seA; p.seB = g.seB;
  p.alpha = g.alpha; p.beta = g.beta;
  p.batch = g.batch;
  p.split = (g.split_k > 1 && g.ws) ? g.split_k : 1;
  p.kbchunk = p.split > 1 ? ceil_div(g.KB, p.split) : (g.KB > 0 ? g.KB : 1);
  if (p.split > 1) p.split = ceil_div(g.KB, p.kbchunk);
  p.ws = g.ws;
  p.eA0 = g.eA0; p.eB0 = g.eB0;
  p.sxs = g.stream_step; p.sxg = g.stream_group_step;
  p.sgsh = g.stream_gs == 8 ? 3 : 4;
  p.avoid = g.avoid_word;
  p.nxcd = g.avoid_xcds;
  if (p.avoid && (!t256 || !p.counter))
    throw std::invalid_argument("gemm_x3p: avoid_word needs a 256-tile launch with a tile counter");
  return p;
}

static void x3p_reduce(hipStream_t s, const PParams &p) {
  if (p.split <= 1) return;
  const long tot = (long)p.batch * p.M * p.N;
  hipLaunchKernelGGL(x3p_splitk_reduce, dim3((int)std::min<long>(2048, (tot + 255) / 256)), dim3(256), 0, s, p);
}

void gemm_x3p(hipStream_t s, const X3PArgs &g) {
  if (g.M <= 0 || g.N <= 0 || g.batch <= 0) return;
  if (g.producer.lines && !rnn_side_gated(s))
    throw std::logic_error("gemm_x3p: streaming launch beside a recurrence without its residency gate");
  bool t256 = false;
  PParams p = x3p_params(g, t256);
  const int total = p.tiles * p.batch * p.split;
  int blocks = total;
  if (g.max_blocks > 0 && total > g.max_blocks) blocks = std::max(8, g.max_blocks / 8 * 8);
  if (g.producer.lines && g.stream_arrive && g.stream_part && g.KB % 2 == 0 && (long)g.M * g.ldc * 4 + (long)(g.batch - 1) * g.sC * 4 < (1L << 31)) {
    p.sdir = 1;
    p.kbchunk = g.KB / 2;  // the producer's two directions
    p.arrive = g.stream_arrive;
    p.part = g.stream_part;
    KCTC_HIP_CHECK(hipMemsetAsync(p.arrive, 0, sizeof(int) * (size_t)stream_total(p) / 2, s));
  }
  if (p.counter) KCTC_HIP_CHECK(hipMemsetAsync(p.counter, 0, sizeof(int), s));
  if (t256) {
    if (g.bf16 && (p.eA || p.eB)) throw std::invalid_argument("gemm_x3p: bf16 operands take no exponents");
    if (g.bf16) x3p_launch<gemm_p256_kernel<true>>(dim3(blocks), NTH2, kLds256, s, p);
    else x3p_launch<gemm_p256_kernel<false>>(dim3(blocks), NTH2, kLds256, s, p);
  } else if (g.bf16 && !p.sflags) {
    if (p.eA || p.eB) throw std::invalid_argument("gemm_x3p: bf16 operands take no exponents");
    x3p_launch<gemm_x3p_kernel<false, true>>(dim3(blocks), NTH, kLdsBase, s, p);
  } else if (p.sflags) {
    if (!p.counter || p.split > 1 || g.stream_N <= 0 || g.stream_step <= 0 ||
        (long)g.stream_T * g.stream_step * 2 >= (1L << 31))
      throw std::invalid_argument("gemm_x3p: bad streaming arguments");
    // persistent blocks, each owning its CU's LDS, so the producer's
    // workgroups always find free CUs (producer.blocks = CUs left to this GEMM)
    const int sb = std::min(stream_total(p), g.producer.blocks > 0 ? g.producer.blocks : 176);
    if (g.bf16) {  // A: the producer's bf16 h images (same chunk addressing, 64 k per block)
      if (p.eB) throw std::invalid_argument("gemm_x3p: bf16 operands take no exponents");
      x3p_launch<gemm_x3p_kernel<true, true>>(dim3(sb), NTH, kLdsStream, s, p);
    } else {
      x3p_launch<gemm_x3p_kernel<true>>(dim3(sb), NTH, kLdsStream, s, p);
    }
    return;
  } else {
    x3p_launch<gemm_x3p_kernel<false>>(dim3(blocks), NTH, kLdsBase, s, p);
  }
  x3p_reduce(s, p);
}

void gemm_x3p_pair(hipStream_t s, const X3PArgs &g1, const X3PArgs &g2) {
  if (g2.M <= 0 || g2.N <= 0 || g2.batch <= 0) return gemm_x3p(s, g1);
  if (g1.M <= 0 || g1.N <= 0 || g1.batch <= 0) return gemm_x3p(s, g2);
  bool a = false, b = false;
  PParams p = x3p_params(g1, a), q = x3p_params(g2, b);
  if (!a || !b || !p.counter || g1.bf16 != g2.bf16 || g1.producer.lines || g2.producer.lines)
    throw std::invalid_argument("gemm_x3p_pair: two 256-tile problems with a tile counter");
  if (g1.bf16 && (p.eA || p.eB || q.eA || q.eB)) throw std::invalid_argument("gemm_x3p: bf16 operands take no exponents");
  const int total = p.tiles * p.batch * p.split + q.tiles * q.batch * q.split;
  int blocks = total;
  if (g1.max_blocks > 0 && total > g1.max_blocks) blocks = std::max(8, g1.max_blocks / 8 * 8);
  KCTC_HIP_CHECK(hipMemsetAsync(p.counter, 0, sizeof(int), s));
  if (g1.bf16) x3p_launch<gemm_p256_pair_kernel<true>>(dim3(blocks), NTH2, kLds256, s, p, q);
  else x3p_launch<gemm_p256_pair_kernel<false>>(dim3(blocks), NTH2, kLds256, s, p, q);
  x3p_reduce(s, p);
  x3p_reduce(s, q);
}

}  // namespace kctc
