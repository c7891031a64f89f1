// seq_align.hip -- the kernels of the length-aware inference and training paths (gfx950).
//
// A batch of N sequences of lengths len[n] <= T runs through the unchanged
// persistent recurrences, which know nothing of lengths.  The forward
// direction is causal: what follows a sequence's last frame cannot reach its
// real frames.  The reverse direction starts at row T-1 with zero state, so
// every sequence must END there: its gate pre-activations G (the reverse
// direction's columns) are shifted right by T - len[n] frames before the
// recurrence, and that direction's output is shifted back after it
// (k_seq_shift, one pass each, 16-byte accesses, no atomics).  Padding rows
// are written as zeros on both sides.  Training (rnn.h rnn_forward_training_seq)
// uses the same map twice more: dy enters the backward recurrence aligned like
// G (forward columns masked, reverse columns shifted right), and the dGates
// images E / DX leave it un-aligned like y, both in one launch.
//
// Decode side: k_blank_scan_batch / k_decodable_rows_batch build the
// CtcDecodableAmNnet matrix (decodable.hip has the arithmetic) of N utterances
// at once (one workgroup per utterance; the "none kept, then keep all" rule
// per utterance, ctc-decodable-am-nnet.cc:52-68; a single utterance is N = 1), and
// k_post_sum_slabs / k_post_sum_reduce the masked column sum behind the
// average-posterior priors (matrix-sum-rows | vector-sum of the recipe).
#include "seq_align.h"

#include <algorithm>

#include "common.h"
#include "prof.h"

namespace kctc {

bool seq_lens(const int *host_lens, int T, int N, SeqLens *out) {
  if (!host_lens || N <= 0 || N > kSeqMaxN || T <= 0) return false;
  for (int n = 0; n < kSeqMaxN; n++) out->len[n] = 0;
  for (int n = 0; n < N; n++) {
    if (host_lens[n] < 1 || host_lens[n] > T) return false;
    out->len[n] = host_lens[n];
  }
  return true;
}

namespace {

// V: float4 (W, Wfwd multiples of 4, 16-byte aligned buffers) or float.
// One element of V per thread and grid-stride step; Wv / Wfv in units of V.
// blockIdx.y picks the image: (src, dst) or, one launch for two images of the
// same shape (a GRU's E and DX), (src2, dst2).
template <typename V, bool kUnalign>
__global__ __launch_bounds__(256) void k_seq_shift(const V *__restrict__ src, V *__restrict__ dst,
                                                   const V *__restrict__ src2, V *__restrict__ dst2, int T, int N,
                                                   int Wv, int Wfv, SeqLens lens, long total) {
  __shared__ int sl[kSeqMaxN];
  if (threadIdx.x < kSeqMaxN) sl[threadIdx.x] = lens.len[threadIdx.x];
  __syncthreads();
  if (blockIdx.y) { src = src2; dst = dst2; }
  const long step = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
    const long row = i / Wv;
    const int c = (int)(i - row * Wv);
    const int t = (int)(row / N), n = (int)(row - (long)t * N);
    const int L = sl[n];
    long from = -1;  // source row (none: zero)
    if (c < Wfv) {
      if (t < L) from = row;
    } else if (kUnalign) {
      if (t < L) from = (long)(t + (T - L)) * N + n;
    } else {
      if (t >= T - L) from = (long)(t - (T - L)) * N + n;
    }
    V v{};
    if (from >= 0) v = src[from * Wv + c];
    dst[i] = v;
  }
}

// The training passes (tag given) cap the grid at 8 blocks per CU and
// grid-stride the rest; the inference passes keep their launch.
constexpr long kTrainGridCap = 2048;

template <bool kUnalign>
void launch_shift(hipStream_t s, const float *src, float *dst, int T, int N, int W, int Wfwd, const SeqLens &lens,
                  const char *tag = nullptr, const float *src2 = nullptr, float *dst2 = nullptr) {
  if (T <= 0 || N <= 0 || W <= 0) return;
  const bool two = src2 && dst2;
  uintptr_t bits = (uintptr_t)src | (uintptr_t)dst;
  if (two) bits |= (uintptr_t)src2 | (uintptr_t)dst2;
  const bool v4 = W % 4 == 0 && Wfwd % 4 == 0 && bits % 16 == 0;
  const int e = v4 ? 4 : 1;
  const long total = (long)T * N * (W / e);
  const unsigned grid = (unsigned)std::min<long>((total + 255) / 256, tag ? kTrainGridCap : 1L << 16);
  ProfSpan ps(s, tag ? tag : kUnalign ? "seq_unalign" : "seq_align");
  if (v4)
    hipLaunchKernelGGL((k_seq_shift<float4, kUnalign>), dim3(grid, two ? 2 : 1), dim3(256), 0, s,
                       reinterpret_cast<const float4 *>(src), reinterpret_cast<float4 *>(dst),
                       reinterpret_cast<const float4 *>(src2), reinterpret_cast<float4 *>(dst2), T, N, W / 4,
                       Wfwd / 4, lens, total);
  else
    hipLaunchKernelGGL((k_seq_shift<float, kUnalign>), dim3(grid, two ? 2 : 1), dim3(256), 0, s, src, dst, src2, dst2,
                       T, N, W, Wfwd, lens, total);
  KCTC_HIP_CHECK(hipGetLastError());
}

// dst[t*N+n] = index of frame t among utterance n's kept frames (or -1);
// kept[n] = their count.  Workgroup n scans its len[n] flags in frame order.
__global__ __launch_bounds__(1024) void k_blank_scan_batch(const float *__restrict__ probs, int N, int A, SeqLens lens,
                                                           float blank_threshold, int *__restrict__ dst,
                                                           int *__restrict__ kept) {
  __shared__ int wsum[16];
  __shared__ int base;
  const int n = blockIdx.x, T = lens.len[n];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const bool skip = blank_threshold < 1.0f;
  if (tid == 0) base = 0;
  __syncthreads();
  for (int c0 = 0; c0 < T; c0 += 1024) {
    const int t = c0 + tid;
    const long r = (long)t * N + n;
    const int k = (t < T) && (!skip || probs[r * A] < blank_threshold) ? 1 : 0;
    int v = k;  // inclusive scan within the wave, then across the 16 waves
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(v, o, 64);
      if (lane >= o) v += u;
    }
    if (lane == 63) wsum[w] = v;
    __syncthreads();
    int off = base;
    for (int i = 0; i < w; i++) off += wsum[i];
    if (t < T) dst[r] = k ? off + v - 1 : -1;
    __syncthreads();
    if (tid == 1023) base = off + v;
    __syncthreads();
  }
  const bool none = skip && base == 0;  // "No Frame will be keeped ..., don't skip blank"
  if (none)
    for (int t = tid; t < T; t += 1024) dst[(long)t * N + n] = t;
  if (tid == 0) kept[n] = none ? T : base;
}

// one wave per frame (t, n): gather, floor, log, prior, scale into the row
// kept[0] + ... + kept[n-1] + dst[t*N+n] of out
__global__ __launch_bounds__(256) void k_decodable_rows_batch(const float *__restrict__ probs, long rows, int N, int A,
                                                              SeqLens lens, const int *__restrict__ dst,
                                                              const int *__restrict__ kept,
                                                              const float *__restrict__ priors, float prob_scale,
                                                              float floor_v, float *__restrict__ out) {
  __shared__ int sl[kSeqMaxN];
  if (threadIdx.x < kSeqMaxN) sl[threadIdx.x] = lens.len[threadIdx.x];
  __syncthreads();
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= rows) return;
  const int t = (int)(r / N), n = (int)(r - (long)t * N);
  if (t >= sl[n]) return;
  const int d = dst[r];
  if (d < 0) return;
  int before = lane < n ? kept[lane] : 0;  // N <= 64
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) before += __shfl_xor(before, o, kWave);
  const float *p = probs + r * A;
  float *o = out + ((long)before + d) * A;
  for (int j = lane; j < A; j += 64) {
    float v = logf(fmaxf(p[j], floor_v));
    if (priors) v += -1.0f * logf(priors[j]);
    o[j] = v * prob_scale;
  }
}

constexpr int kSlabRows = 64;

// partial[b][a] = sum over the real rows of slab b (rows b*64 .. +63, in row
// order) of m[row][a]; thread j owns columns j, j+256, ...
__global__ __launch_bounds__(256) void k_post_sum_slabs(const float *__restrict__ m, long rows, int N, int A,
                                                        SeqLens lens, double *__restrict__ partial) {
  __shared__ int sl[kSeqMaxN];
  if (threadIdx.x < kSeqMaxN) sl[threadIdx.x] = lens.len[threadIdx.x];
  __syncthreads();
  const long r0 = (long)blockIdx.x * kSlabRows, r1 = r0 + kSlabRows < rows ? r0 + kSlabRows : rows;
  for (int a = threadIdx.x; a < A; a += 256) {
    double acc = 0.0;
    for (long r = r0; r < r1; r++) {
      const int t = (int)(r / N), n = (int)(r - (long)t * N);
      if (t < sl[n]) acc += (double)m[r * A + a];
    }
    partial[(long)blockIdx.x * A + a] = acc;
  }
}
// sum[a] += partial[0][a] + partial[1][a] + ... (slab order)
__global__ __launch_bounds__(256) void k_post_sum_reduce(const double *__restrict__ partial, int slabs, int A,
                                                         double *__restrict__ sum) {
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (a >= A) return;
  double acc = 0.0;
  for (int b = 0; b < slabs; b++) acc += partial[(long)b * A + a];
  sum[a] += acc;
}

}  // namespace

void seq_align(hipStream_t s, const float *src, float *dst, int T, int N, int W, int Wfwd, const SeqLens &lens) {
  launch_shift<false>(s, src, dst, T, N, W, Wfwd, lens);
}
void seq_unalign(hipStream_t s, const float *src, float *dst, int T, int N, int W, int Wfwd, const SeqLens &lens) {
  launch_shift<true>(s, src, dst, T, N, W, Wfwd, lens);
}

void seq_align_dy(hipStream_t s, const float *dy, float *dst, int T, int N, int W, int Wfwd, const SeqLens &lens) {
  launch_shift<false>(s, dy, dst, T, N, W, Wfwd, lens, "seq_align_dy");
}
void seq_unalign_dgates(hipStream_t s, const float *e_src, float *e_dst, const float *dx_src, float *dx_dst, int T,
                        int N, int W, int Wfwd, const SeqLens &lens) {
  const bool two = dx_src && dx_src != e_src;
  launch_shift<true>(s, e_src, e_dst, T, N, W, Wfwd, lens, "seq_unalign_dgates", two ? dx_src : nullptr,
                     two ? dx_dst : nullptr);
}
void seq_align_train(hipStream_t s, const float *src, float *dst, int T, int N, int W, int Wfwd,
                     const SeqLens &lens) {
  launch_shift<false>(s, src, dst, T, N, W, Wfwd, lens, "seq_align_train");
}
void seq_unalign_train(hipStream_t s, const float *src, float *dst, int T, int N, int W, int Wfwd,
                       const SeqLens &lens) {
  launch_shift<true>(s, src, dst, T, N, W, Wfwd, lens, "seq_unalign_train");
}

size_t seq_decodable_scratch_bytes(int T, int N) { return sizeof(int) * ((size_t)T * N + 64); }

void seq_decodable(hipStream_t s, const float *probs, int T, int N, int A, const SeqLens &lens, const float *priors,
                   float prob_scale, float blank_threshold, float floor_v, float *out, void *scratch, int *kept_dev) {
  if (T <= 0 || N <= 0 || N > kSeqMaxN || A <= 0) return;
  int *dst = static_cast<int *>(scratch);
  const long rows = (long)T * N;
  ProfSpan ps(s, "seq_decodable");
  hipLaunchKernelGGL(k_blank_scan_batch, dim3(N), dim3(1024), 0, s, probs, N, A, lens, blank_threshold, dst, kept_dev);
  hipLaunchKernelGGL(k_decodable_rows_batch, dim3(ceil_div(rows, 4)), dim3(256), 0, s, probs, rows, N, A, lens, dst,
                     kept_dev, priors, prob_scale, floor_v, out);
  KCTC_HIP_CHECK(hipGetLastError());
}

size_t seq_post_sum_scratch_bytes(int T, int N, int A) {
  return sizeof(double) * (size_t)ceil_div((long)T * N, kSlabRows) * A;
}

void seq_post_sum(hipStream_t s, const float *m, int T, int N, int A, const SeqLens &lens, double *sum, void *scratch) {
  if (T <= 0 || N <= 0 || N > kSeqMaxN || A <= 0) return;
  const long rows = (long)T * N;
  const int slabs = ceil_div(rows, kSlabRows);
  double *partial = static_cast<double *>(scratch);
  ProfSpan ps(s, "post_sum");
  hipLaunchKernelGGL(k_post_sum_slabs, dim3(slabs), dim3(256), 0, s, m, rows, N, A, lens, partial);
  hipLaunchKernelGGL(k_post_sum_reduce, dim3(ceil_div(A, 256)), dim3(256), 0, s, partial, slabs, A, sum);
  KCTC_HIP_CHECK(hipGetLastError());
}

}  // namespace kctc
