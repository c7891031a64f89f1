// seq_align.h -- kernels of the length-aware (variable-length batch) inference
// path (seq_align.hip): the time shift that lets the unchanged recurrences run
// the reverse direction of N sequences of different lengths, the batched
// blank-skip compaction of CtcDecodableAmNnet, and the masked posterior sum.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace kctc {

constexpr int kSeqMaxN = 64;  // sequences per batch (rec_common.h kMaxRT: N <= 64)

// The host lengths travel as a kernel argument: consumed by the launch call,
// no staging copy and no host synchronisation.
struct SeqLens {
  int len[kSeqMaxN];
};
// false when N or a length is out of range ([1, T])
bool seq_lens(const int *host_lens, int T, int N, SeqLens *out);

// Rows are time-major, row t*N+n of W floats; src and dst are distinct buffers.
// Columns [0, Wfwd) (forward direction: causal, unshifted):
//   dst[t,n] = t < len[n] ? src[t,n] : 0
// Columns [Wfwd, W) (reverse direction), with shift = T - len[n]:
//   seq_align   dst[t,n] = t >= shift ? src[t-shift, n] : 0    (padding first)
//   seq_unalign dst[t,n] = t < len[n] ? src[t+shift, n] : 0    (shifted back)
// Rows t >= len[n] of src are never read by seq_align.
void seq_align(hipStream_t s, const float *src, float *dst, int T, int N, int W, int Wfwd, const SeqLens &lens);
void seq_unalign(hipStream_t s, const float *src, float *dst, int T, int N, int W, int Wfwd, const SeqLens &lens);
// The passes of length-aware training, the same two maps under profile names
// of their own and a grid capped at 8 blocks per CU (grid-stride beyond):
//   seq_align_train / seq_unalign_train  G in, y out of the forward
//   seq_align_dy        dy into the backward recurrence (padding rows of dy
//                       may hold anything finite: never read)
//   seq_unalign_dgates  the backward recurrence's dGates images out of their
//                       scratch: E and (a GRU; else null or == e_src) DX, both
//                       [T*N][W], in ONE launch; padding rows become +0
void seq_align_train(hipStream_t s, const float *src, float *dst, int T, int N, int W, int Wfwd, const SeqLens &lens);
void seq_unalign_train(hipStream_t s, const float *src, float *dst, int T, int N, int W, int Wfwd,
                       const SeqLens &lens);
void seq_align_dy(hipStream_t s, const float *dy, float *dst, int T, int N, int W, int Wfwd, const SeqLens &lens);
void seq_unalign_dgates(hipStream_t s, const float *e_src, float *e_dst, const float *dx_src, float *dx_dst, int T,
                        int N, int W, int Wfwd, const SeqLens &lens);

// CtcDecodableAmNnet over a batch: probs [T*N][A] time-major (the output of a
// model ending in SoftmaxComponent), utterance n has frames t < len[n].  The
// kept frames of utterance 0, then of utterance 1, ... go to out [sum kept][A]
// (capacity sum len); kept_dev[n] = rows of utterance n.  Per utterance the
// rule of decodable.hip: frames with probs[t][0] < blank_threshold, or all of
// its frames when none qualifies.  scratch: seq_decodable_scratch_bytes(T, N).
size_t seq_decodable_scratch_bytes(int T, int N);
void seq_decodable(hipStream_t s, const float *probs, int T, int N, int A, const SeqLens &lens, const float *priors,
                   float prob_scale, float blank_threshold, float floor_v, float *out, void *scratch, int *kept_dev);

// sum[a] += sum over the real frames (t < len[n]) of m[t*N+n][a], fp64, in a
// fixed order (row slabs in row order, then the slabs in slab order): the
// result does not depend on the launch.  scratch: seq_post_sum_scratch_bytes.
size_t seq_post_sum_scratch_bytes(int T, int N, int A);
void seq_post_sum(hipStream_t s, const float *m, int T, int N, int A, const SeqLens &lens, double *sum, void *scratch);

}  // namespace kctc
