/*
 * ctc.h -- warp-ctc compatible C ABI, implemented by libkaldictc_amd.so with
 * hand-written CDNA4 (gfx950) HIP kernels.
 *
 * Replaces the external warp-ctc library that the reference includes as
 *     extern "C" { #include "ctc.h" }          src/ctc/ctc-nnet-update.cc:27-29
 * and calls as
 *     get_workspace_size(...)                  src/ctc/ctc-nnet-update.cc:211-214
 *     compute_ctc_loss(...)  (grads / NULL)    src/ctc/ctc-nnet-update.cc:224-243
 *     ctcGetStatusString(ret)                  src/ctc/ctc-nnet-update.cc:31-37
 * The declarations reproduce the public upstream warp-ctc API (baidu-research
 * warp-ctc include/ctc.h, which the lifeiteng fork installed by
 * tools/extras/install_warp_ctc.sh:8-11 keeps); CUstream becomes hipStream_t.
 *
 * Contract (unchanged from warp-ctc):
 *  - activations [maxT][minibatch][alphabet_size] float, DEVICE, C-order,
 *    maxT = max(input_lengths); un-normalised (softmax is applied inside).
 *  - gradients   same shape, DEVICE, nullable; d(-log p)/d activations.  Rows
 *    t >= input_lengths[n] are written with 0 (the caller need not pre-zero).
 *  - flat_labels, label_lengths, input_lengths, costs: HOST pointers.
 *    costs[n] = -log p(labels_n | x_n), filled when the call returns (the call
 *    synchronises options.stream).  An utterance with L + repeats > T gets
 *    cost 0 and a zero gradient (warp-ctc's CPU behaviour).
 *  - workspace: DEVICE, >= get_workspace_size() bytes, owned by the caller.
 *  - loc must be CTC_GPU: this build has no CPU compute path (a CTC_CPU call
 *    returns CTC_STATUS_INVALID_VALUE).
 */
#ifndef KALDI_CTC_AMD_CTC_H_
#define KALDI_CTC_AMD_CTC_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

struct ihipStream_t;
typedef struct ihipStream_t *ctcStream_t; /* == hipStream_t */

typedef enum {
  CTC_STATUS_SUCCESS = 0,
  CTC_STATUS_MEMOPS_FAILED = 1,
  CTC_STATUS_INVALID_VALUE = 2,
  CTC_STATUS_EXECUTION_FAILED = 3,
  CTC_STATUS_UNKNOWN_ERROR = 4
} ctcStatus_t;

typedef enum { CTC_CPU = 0, CTC_GPU = 1 } ctcComputeLocation;

struct ctcOptions {
  ctcComputeLocation loc;
  union {
    unsigned int num_threads; /* CTC_CPU (unsupported here) */
    ctcStream_t stream;       /* CTC_GPU */
  };
  int blank_label;
};

int get_warpctc_version(void);
const char *ctcGetStatusString(ctcStatus_t status);

ctcStatus_t compute_ctc_loss(const float *const activations, float *gradients,
                             const int *const flat_labels, const int *const label_lengths,
                             const int *const input_lengths, int alphabet_size,
                             int minibatch, float *costs, void *workspace,
                             struct ctcOptions options);

ctcStatus_t get_workspace_size(const int *const label_lengths,
                               const int *const input_lengths, int alphabet_size,
                               int minibatch, struct ctcOptions info,
                               size_t *size_bytes);

/* ---- extensions (not in upstream warp-ctc) ------------------------------
 * Stream-ordered variant used by the native trainer: identical math, but
 * costs_dev (double[minibatch], DEVICE) is written asynchronously and the
 * call never synchronises, so a whole train step can be captured/queued
 * without host round trips.  Host arrays are consumed before return. */
ctcStatus_t mictc_compute_ctc_loss_async(const float *activations, float *gradients,
                                         const int *flat_labels, const int *label_lengths,
                                         const int *input_lengths, int alphabet_size,
                                         int minibatch, double *costs_dev, void *workspace,
                                         ctcStream_t stream, int blank_label);

/* TEST / TUNING KNOB, not part of the warp-ctc contract: frames per barrier
 * of the alpha/beta recursion (1..8, larger values clamped; default 8).
 * PROCESS-GLOBAL: every later launch from any thread or
 * network reads it, so set it only while no CTC call is in flight (the tests
 * do, one process).  Returns the previous value; m <= 0 only queries.  Same
 * results for every m (tests/test_ctc_gpu.py). */
int mictc_set_frame_group(int m);

/* TEST KNOB, not part of the warp-ctc contract: 1 (default) runs the
 * alpha/beta recursion on overlapping per-wave state windows wherever their
 * 12 waves hold the longest label sequence, and on the long-label kernel (512
 * threads, 3 states per thread, one barrier per frame) beyond that; 0 runs
 * the long-label kernel for every batch, so that the tests reach it at small
 * sizes too.  Process-global like mictc_set_frame_group; same results either
 * way (tests/test_ctc_gpu.py).  Returns the previous value; on < 0 only
 * queries. */
int mictc_set_win(int on);

/* ---- CTC forced alignment (Viterbi; csrc/ctc_align.hip) -------------------
 * The best path of each utterance through its own transcript: with
 * lp[t][a] the log-softmax of frame t and l' the blank-interleaved labels
 * (S = 2L+1 states, even ones blank),
 *   v_0(0) = lp[0][blank], v_0(1) = lp[0][l'_1], the rest -inf;
 *   v_t(s) = lp[t][l'_s] + max(v_{t-1}(s), v_{t-1}(s-1), v_{t-1}(s-2)),
 * the last candidate only for odd s >= 2 with l'_s != l'_{s-2}.  A later
 * candidate wins only if it is strictly greater (staying beats a step of one
 * beats a skip); the path ends in state S-1 unless state S-2 scores strictly
 * higher.
 *  - activations [maxT][minibatch][alphabet_size] float, DEVICE, un-normalised,
 *    maxT = max(input_lengths); rows t >= input_lengths[n] are never read
 *    (they may hold NaN).
 *  - flat_labels, label_lengths, input_lengths: HOST, consumed before return.
 *  - ali_dev int [maxT][minibatch], DEVICE: row t*minibatch+n is the symbol
 *    (blank included) of frame t of utterance n, -1 for t >= input_lengths[n].
 *  - scores_dev double [minibatch], DEVICE: log-probability of that path.
 *  - An utterance with T == 0 or L + repeats > T gets all -1 and score -inf;
 *    L == 0 gives the all-blank path.
 *  - workspace: DEVICE, >= mictc_get_align_workspace_size() bytes (it holds
 *    the normalised log-probs and 2 bits of back-pointer per frame and state).
 * Stream-ordered: never synchronises, allocates no device memory.  Invalid
 * lengths, L > 639, a label out of range or equal to blank_label and null
 * pointers return CTC_STATUS_INVALID_VALUE and enqueue nothing.
 * Deterministic (no atomics). */
ctcStatus_t mictc_get_align_workspace_size(const int *label_lengths, const int *input_lengths,
                                           int alphabet_size, int minibatch, size_t *size_bytes);
ctcStatus_t mictc_ctc_align_async(const float *activations, const int *flat_labels,
                                  const int *label_lengths, const int *input_lengths,
                                  int alphabet_size, int minibatch, int *ali_dev, double *scores_dev,
                                  void *workspace, ctcStream_t stream, int blank_label);

/* TEST KNOB: 1 (default) runs the Viterbi recursion with one state per thread
 * wherever 512 threads hold the longest label sequence (S <= 512) and with 512
 * threads of 3 states beyond; 0 runs the 3-state kernel for every batch, so
 * that the tests reach it at small sizes.  Process-global like mictc_set_win;
 * same results either way (tests/test_ctc_align_gpu.py).  Returns the
 * previous value; on < 0 only queries. */
int mictc_set_align_kernel(int on);

/* ---- CTC prefix beam search (lexicon-free; csrc/ctc_beam.hip) --------------
 * The most likely transcript of each utterance among the prefixes a beam
 * keeps.  With lp[t][a] the log-softmax of frame t, a prefix p (a sequence of
 * non-blank labels, last label e) carries over frames 0..t
 *   b(p):  log-prob of the alignments that collapse to p and end in blank,
 *   nb(p): the same for those that end in a label;  tot = b (+) nb (log-add).
 * Before frame 0 the beam holds the empty prefix with b = 0, nb = -inf.
 * Frame t, with C_t the K = min(symbols, alphabet_size - 1) non-blank symbols
 * of largest lp[t][c] (ties to the lower id):
 *   stay    b'(p)  (+)= lp[t][blank] + tot(p);
 *           nb'(p) (+)= lp[t][e] + nb(p)                      (p non-empty);
 *   extend  nb'(p+c) (+)= lp[t][c] + (c == e ? b(p) : tot(p))  for c in C_t;
 *   merge   prefixes that are equal as label sequences are one entry and their
 *           contributions add (p+c may already be in the beam);
 *   prune   the `beam` entries of largest tot' stay (ties: deterministic).
 * The result is the entry of largest tot after the last frame.
 *  - activations [maxT][minibatch][alphabet_size] float, DEVICE, un-normalised,
 *    maxT = max(input_lengths); rows t >= input_lengths[n] are never read.
 *  - input_lengths: HOST, consumed before return; each in [0, maxT].
 *  - hyp_dev int [minibatch][maxT], DEVICE: row n holds the labels of
 *    utterance n, then -1.  hyp_len_dev int [minibatch]: their number.
 *  - scores_dev double [minibatch], DEVICE: tot of the result.  It is a lower
 *    bound of the CTC log-probability of the returned labels (pruning only
 *    drops mass) and equal to it when nothing was pruned.
 *  - An utterance with T == 0 gives length 0 and score 0.
 *  - workspace: DEVICE, >= mictc_get_beam_workspace_size() bytes (the
 *    normalised log-probs and 16 bytes per frame and beam entry of prefix
 *    nodes).
 * 1 <= beam <= 128, 1 <= symbols <= 64, alphabet_size >= 2,
 * 0 <= blank_label < alphabet_size; anything else, a negative length or a
 * null pointer returns CTC_STATUS_INVALID_VALUE and enqueues nothing.
 * Stream-ordered: never synchronises, allocates no device memory.
 * Deterministic (no atomics): two calls give identical bytes. */
ctcStatus_t mictc_get_beam_workspace_size(const int *input_lengths, int alphabet_size, int minibatch,
                                          int beam, size_t *size_bytes);
ctcStatus_t mictc_ctc_beam_search_async(const float *activations, const int *input_lengths,
                                        int alphabet_size, int minibatch, int beam, int symbols,
                                        int *hyp_dev /* [minibatch][maxT], -1 padded */,
                                        int *hyp_len_dev /* [minibatch] */, double *scores_dev /* [minibatch] */,
                                        void *workspace, ctcStream_t stream, int blank_label);

#ifdef __cplusplus
}
#endif
#endif /* KALDI_CTC_AMD_CTC_H_ */
