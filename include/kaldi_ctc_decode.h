/*
 * kaldi_ctc_decode.h -- the decode-side use of a trained CTC model and the
 * validation objective, as a C ABI over gfx950 kernels
 * (csrc/decodable.hip) and the nnet2 trainer's forward pass.
 *
 *   kctc_softmax_rows        <- SoftmaxComponent::Propagate
 *                               (src/nnet2/nnet-component.cc:929-946; the
 *                               component steps/ctc/train.sh:471-477 appends
 *                               for decoding)
 *   kctc_ctc_decodable       <- CtcDecodableAmNnet's log-likelihood matrix
 *                               (src/ctc/ctc-decodable-am-nnet.cc:28-80)
 *   kctc_nnet_propagate      <- NnetComputation (src/nnet2/nnet-compute.cc),
 *                               N time-major sequences
 *   kctc_am_nnet_decodable   <- CtcDecodableAmNnet(trans_model, am_nnet, feats,
 *                               pad_input, prob_scale, blank_threshold)
 *   kctc_nnet_compute_prob   <- nnet2-ctc-compute-prob
 *                               (src/ctcbin/nnet2-ctc-compute-prob.cc:27-111)
 *   kctc_nnet_propagate_seq / kctc_am_nnet_decodable_batch
 *                            <- the two above for N utterances of different
 *                               lengths in one batch (an extension)
 *   kctc_nnet_sum_posteriors <- nnet-ctc-compute-from-egs | matrix-sum-rows |
 *                               vector-sum (steps/ctc/train.sh:469-510)
 *   kctc_am_nnet_adjust_priors <- nnet-adjust-priors
 *   kctc_nnet_insert         <- nnet-insert (src/nnet2/nnet-functions.cc:39-55)
 *   kctc_nnet_align / kctc_nnet_align_egs
 *                            <- CTC forced alignment of a batch / an egs archive
 *                               (an extension; writes the Int32Vector table that
 *                               nnet-ctc-relabel-egs reads)
 *   kctc_nnet_decode / kctc_nnet_decode_egs
 *                            <- lexicon-free CTC prefix beam search of a batch /
 *                               an egs archive (an extension; no WFST)
 * Return 0 on success (kctc_last_error() describes a failure).
 */
#ifndef KALDI_CTC_AMD_KALDI_CTC_DECODE_H_
#define KALDI_CTC_AMD_KALDI_CTC_DECODE_H_

#include <stddef.h>

#include "kaldi_ctc_train.h"

#ifdef __cplusplus
extern "C" {
#endif

struct ihipStream_t;

/* out[r] = softmax(in[r]) (max-subtracted), floored at 1e-20; device, row-major */
int kctc_softmax_rows(struct ihipStream_t *stream, const float *in, long rows, int cols, float *out);

/* probs [T][A] (device; the output of a model ending in SoftmaxComponent) ->
 * out [*num_kept][A] (device):
 *   blank_threshold < 1: only frames t with probs[t][0] < blank_threshold, in
 *     order (all frames if none qualifies, as the reference warns and does);
 *   v = log(max(p, floor_value))   (1e-10 CtcDecodableAmNnet, 1e-20 ...Parallel)
 *   v -= log(priors[a])            (priors: linear, device, nullable)
 *   v *= prob_scale
 * scratch: kctc_ctc_decodable_scratch_bytes(T) bytes of device memory.
 * Synchronises the stream to return *num_kept. */
size_t kctc_ctc_decodable_scratch_bytes(int T);
int kctc_ctc_decodable(struct ihipStream_t *stream, const float *probs, int T, int A, const float *priors,
                       float prob_scale, float blank_threshold, float floor_value, float *out, void *scratch,
                       int *num_kept);

/* forward pass of the whole network: feats_dev [T_max*N*num_splice][input_dim]
 * (FormatNnetInput layout, num_splice = 1 + left + right context,
 * kctc_nnet_context; the caller's buffer must hold that many rows) ->
 * out_dev [T_max*N][output_dim] (device), len = T_max*N*output_dim */
int kctc_nnet_propagate(kctcNnet_t nnet, const float *feats_dev, int T_max, int N, float *out_dev, long len);

/* CtcDecodableAmNnet for one utterance feats_dev [T][input_dim] (plain
 * feature rows) with the model's priors (an nnet2-ctc model file read by
 * kctc_am_nnet_read), pad_input = true (the reference's default): a network
 * with frame context sees the first / last frame repeated LeftContext /
 * RightContext times (NnetComputer, src/nnet2/nnet-compute.cc:64-90), so T
 * frames give T rows.  Writes the kept rows of the [T][A] log-likelihood
 * matrix to out_host (capacity T*A floats), *num_rows = rows kept. */
int kctc_am_nnet_decodable(kctcNnet_t nnet, const float *feats_dev, int T, float prob_scale,
                           float blank_threshold, float *out_host, int *num_rows);

/* ---- variable-length batches -------------------------------------------------
 * The reference evaluates one utterance at a time (mini_batch = 1): nothing
 * masks its sequences, so in a padded batch the reverse direction of a BLSTM
 * would start on the padding.  Here N utterances of different lengths run as
 * one batch and each gets exactly the rows it would get alone: the RNN
 * components take krnnForwardInferenceSeq's path (kaldi_rnn.h), the other
 * components work row by row.  At most 64 utterances per call.
 *
 * kctc_nnet_propagate_seq: kctc_nnet_propagate with host lengths
 * num_frames[n] in [1, T_max].  Row t*N+n of out_dev (t < num_frames[n]) is
 * row t of utterance n's own kctc_nnet_propagate (N = 1); the rows
 * t >= num_frames[n] mean nothing.  Input rows of the padding frames may
 * hold anything finite.  A DropoutComponent draws one mask for the batch;
 * evaluate with the dropout components removed, as the recipe does. */
int kctc_nnet_propagate_seq(kctcNnet_t nnet, const float *feats_dev, int T_max, int N, const int *num_frames,
                            float *out_dev, long len);

/* kctc_am_nnet_decodable for N utterances at once.  feats_dev
 * [T_max*N][input_dim]: plain feature rows, time-major (frame t of utterance
 * n in row t*N+n, t < num_frames[n]; the other rows anything finite).
 * out_host (capacity sum(num_frames)*A floats) receives the kept rows of
 * utterance 0, then of utterance 1, ...; rows[n] = rows kept of utterance n
 * (per utterance: the frames below blank_threshold, or all of its frames if
 * none is).  A network with frame context goes through kctc_am_nnet_decodable
 * one utterance at a time (every utterance is padded at its own ends). */
int kctc_am_nnet_decodable_batch(kctcNnet_t nnet, const float *feats_dev, int T_max, int N, const int *num_frames,
                                 float prob_scale, float blank_threshold, float *out_host, int *rows);

/* nnet-ctc-compute-from-egs | matrix-sum-rows | vector-sum (steps/ctc/train.sh
 * :469-510): sum[a] = the network's output column a summed over every output
 * frame of every example of the archive (binary "ark:").  The examples run in
 * batches of minibatch_size (1..64) in archive order through the
 * variable-length forward; of each example the first eg.left_context -
 * nnet.LeftContext() rows are dropped and the input is not padded
 * (pad_input = false: NumRows - left - right output frames).  The sum runs
 * over whatever the network outputs (posteriors when it ends in a
 * SoftmaxComponent), in fp64 on the device in a fixed order.  sum: A =
 * output_dim doubles (host); *frames = output frames summed; *num_egs =
 * examples read. */
int kctc_nnet_sum_posteriors(kctcNnet_t nnet, const char *rspecifier, int minibatch_size, double *sum, int A,
                             long *frames, long *num_egs);

/* nnet-adjust-priors (src/nnet2bin/nnet-adjust-priors.cc:126-140).
 * google_prior_const != 0: priors = 1 with priors[0] = the constant (left
 * un-normalised, as the reference does; posterior_sum is not read).
 * Otherwise priors = posterior_sum / sum(posterior_sum), which must be > 0
 * (divided in fp64, stored as float).  No floor is applied: the reference
 * registers --prior-floor and never uses it. */
int kctc_am_nnet_adjust_priors(kctcNnet_t nnet, const double *posterior_sum, int A, float google_prior_const);

/* nnet-insert --randomize-next-component=false (InsertComponents,
 * src/nnet2/nnet-functions.cc:39-55): the components built from the config
 * lines (one per line, initialised from `seed`) are inserted before component
 * insert_at, 0 <= insert_at <= kctc_nnet_num_components (= appended: the
 * Softmax of train.sh:472-478; in the middle: the BLSTM that train.sh:357-384
 * adds every add_layers_period iterations).  The existing components keep
 * their parameters.  Dimensions must chain with both neighbours and a
 * component with frame context must stay first (as kctc_nnet_set_component);
 * on an error nothing changes.  No minibatch may be in flight. */
int kctc_nnet_insert(kctcNnet_t nnet, int insert_at, const char *config, unsigned long long seed);

/* nnet2-ctc-compute-prob over an egs archive (binary "ark:"): examples in
 * batches of 10 in archive order, every example used (no training skip
 * rules), ComputeNnetObjf per batch (forward + CTC + best-path accuracy, no
 * update).  Outputs: examples, total objective (sum of -log p; the CLI prints
 * tot_like / tot_weight), total accuracy, total weight (sum of labels). */
int kctc_nnet_compute_prob(kctcNnet_t nnet, const char *rspecifier, long *num_examples, double *tot_like,
                           double *tot_accuracy, double *tot_weight);

/* ---- CTC forced alignment (an extension; the kernels: ctc.h) -------------------
 * kctc_nnet_align: on which frames does the model place each label of a given
 * transcript.  feats_dev, T_max, N, num_frames as for kctc_nnet_propagate_seq
 * (N <= 64): the variable-length forward, so every utterance is aligned as if
 * it were run alone, then mictc_ctc_align_async on the network's stream with
 * blank 0 and input lengths num_frames (the updater's rule: NumFrames minus
 * the ignored context frames, none here).  The alignment runs on un-normalised
 * activations: of a network that ends in a SoftmaxComponent, on that
 * component's input (same result as without the Softmax).  flat_labels,
 * label_lengths: host, symbol ids (label = pdf + 1).  ali_host: T_max*N ints,
 * row t*N+n the symbol of frame t of utterance n (blank 0 included), -1 for
 * t >= num_frames[n] and for every frame of an utterance whose labels do not
 * fit (L + repeats > T); scores_host: N doubles, the log-probability of each
 * path (-inf: does not fit). */
int kctc_nnet_align(kctcNnet_t nnet, const float *feats_dev, int T_max, int N, const int *num_frames,
                    const int *flat_labels, const int *label_lengths, int *ali_host, double *scores_host);

/* Aligns every example of an egs archive (binary "ark:", read as
 * kctc_nnet_sum_posteriors reads it: batches of minibatch_size (1..64) in
 * archive order, each example from its own start offset) to its own labels
 * and writes, per example key, the alignment as a Kaldi Int32Vector to a
 * binary "ark:" -- the table nnet-ctc-relabel-egs and ali-to-post read.
 * Symbol ids as they are (blank 0, label = pdf + 1).  Examples whose labels do
 * not fit are counted and not written.  Outputs (nullable): examples written,
 * examples that do not fit, the sum of the written paths' log-probabilities
 * and of their frames. */
int kctc_nnet_align_egs(kctcNnet_t nnet, const char *egs_rspecifier, const char *ali_wspecifier,
                        int minibatch_size, long *num_done, long *num_infeasible, double *tot_score, long *tot_frames);

/* ---- CTC prefix beam search (an extension; the kernels and the recursion: ctc.h) ----
 * kctc_nnet_decode: the most likely label sequence of every utterance that a
 * beam of `beam` (1..128) prefixes finds, each frame extending by its
 * `symbols` (1..64) most likely labels.  feats_dev, T_max, N, num_frames as for
 * kctc_nnet_propagate_seq (N <= 64): the variable-length forward, so every
 * utterance is decoded as if it were run alone, then
 * mictc_ctc_beam_search_async on the network's stream with blank 0.  Like the
 * alignment it runs on un-normalised activations: of a network that ends in a
 * SoftmaxComponent, on that component's input.  No priors, no prob-scale, no
 * lexicon.  hyp_host: N*T_max ints, row n the labels of utterance n (symbol
 * ids, label = pdf + 1) then -1; hyp_len_host: N ints; scores_host: N doubles,
 * the log-probability the beam holds for each result. */
int kctc_nnet_decode(kctcNnet_t nnet, const float *feats_dev, int T_max, int N, const int *num_frames, int beam,
                     int symbols, int *hyp_host, int *hyp_len_host, double *scores_host);

/* Decodes every example of an egs archive (read as kctc_nnet_align_egs reads
 * it) and writes, per example key, the hypothesis as a Kaldi Int32Vector to a
 * binary "ark:".  Outputs (nullable): examples decoded, the sum of their own
 * label counts and the sum of LevenshteinEditDistance(labels, hypothesis), so
 * that 1 - edit_distance / num_labels compares with kctc_nnet_compute_prob's
 * best-path accuracy. */
int kctc_nnet_decode_egs(kctcNnet_t nnet, const char *egs_rspecifier, const char *hyp_wspecifier, int minibatch_size,
                         int beam, int symbols, long *num_utts, long *num_labels, long *edit_distance);

#ifdef __cplusplus
}
#endif
#endif /* KALDI_CTC_AMD_KALDI_CTC_DECODE_H_ */
