// decodable.hip -- the decode-side use of a trained CTC model (SURVEY §8f
// row 3): SoftmaxComponent::Propagate (the component the recipe appends
// before decoding, egs/wsj/s5/steps/ctc/train.sh:471-477) and the
// CtcDecodableAmNnet log-likelihood matrix (src/ctc/ctc-decodable-am-nnet.cc:28-80):
//
//   probs = softmax(nnet output), floored at 1e-20     (nnet-component.cc:929-946)
//   if blank_threshold < 1: keep only frames with probs[t][0] < blank_threshold
//     (all of them if none would remain)               (:52-68)
//   log_probs = log(max(probs, floor))                 (:70-71, floor 1e-10;
//                                                       CtcDecodableAmNnetParallel 1e-20)
//   log_probs -= log(priors)   (when the AmNnet has priors)  (:73-79)
//   log_probs *= prob_scale                            (:81-82)
//
// Kernels: k_softmax_rows (one wave per row); the blank scan (one workgroup
// per utterance: ordered compaction of the kept frames, the CopyRows of
// :63-65) and the row kernel (one wave per kept row: gather, floor, log,
// prior, scale) are seq_align.hip's, which take a batch of utterances.
#include "common.h"
#include "decodable.h"
#include "seq_align.h"

namespace kctc {
namespace {

__global__ __launch_bounds__(256) void k_softmax_rows(const float *__restrict__ in, long rows, int cols,
                                                      float *__restrict__ out) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float *x = in + row * cols;
  float m = -INFINITY;
  for (int j = lane; j < cols; j += 64) m = fmaxf(m, x[j]);
  m = wave_max(m);
  float s = 0.f;
  for (int j = lane; j < cols; j += 64) s += expf(x[j] - m);
  s = wave_sum(s);
  const float inv = 1.f / s;
  float *y = out + row * cols;
  for (int j = lane; j < cols; j += 64) y[j] = fmaxf(expf(x[j] - m) * inv, 1.0e-20f);
}

// DiffSoftmaxPerRow (SoftmaxComponent::Backprop, nnet-component.cc:948-976):
// d_i = p_i e_i - p_i (p . e), one wave per row
__global__ __launch_bounds__(256) void k_diff_softmax_rows(const float *__restrict__ p, const float *__restrict__ e,
                                                           long rows, int cols, float *__restrict__ d) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float *pr = p + row * cols, *er = e + row * cols;
  float s = 0.f;
  for (int j = lane; j < cols; j += 64) s += pr[j] * er[j];
  s = wave_sum(s);
  float *dr = d + row * cols;
  for (int j = lane; j < cols; j += 64) dr[j] = pr[j] * (er[j] - s);
}

}  // namespace

void diff_softmax_rows(hipStream_t s, const float *value, const float *deriv, long rows, int cols, float *out) {
  if (rows <= 0 || cols <= 0) return;
  hipLaunchKernelGGL(k_diff_softmax_rows, dim3(ceil_div(rows, 4)), dim3(256), 0, s, value, deriv, rows, cols, out);
}

void softmax_rows(hipStream_t s, const float *in, long rows, int cols, float *out) {
  if (rows <= 0 || cols <= 0) return;
  hipLaunchKernelGGL(k_softmax_rows, dim3(ceil_div(rows, 4)), dim3(256), 0, s, in, rows, cols, out);
}

size_t ctc_decodable_scratch_bytes(int T) { return sizeof(int) * ((size_t)T + 64); }

void ctc_decodable(hipStream_t s, const float *probs, int T, int A, const float *priors, float prob_scale,
                   float blank_threshold, float floor_v, float *out, void *scratch, int *kept_dev) {
  if (T <= 0 || A <= 0) return;
  SeqLens lens{};  // a batch of one utterance (seq_align.hip)
  lens.len[0] = T;
  seq_decodable(s, probs, T, 1, A, lens, priors, prob_scale, blank_threshold, floor_v, out, scratch, kept_dev);
}

}  // namespace kctc
