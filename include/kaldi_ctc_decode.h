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
 *   kctc_graph_* / kctc_wfst_decode_async / kctc_nnet_decode_graph(_egs)
 *                            <- the best path of nnet2-ctc-latgen-faster
 *                               (src/ctcbin/nnet2-ctc-latgen-faster.cc: Viterbi
 *                               token passing over a decoding graph with --beam
 *                               and --max-active; no lattice)
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

/* ---- WFST decoding (kernels: csrc/wfst_decode.hip) ---------------
 * A decoding graph is a weighted finite-state transducer in the tropical
 * semiring: states 0..S-1, a start state, a final cost per state (+inf: not
 * final) and arcs (src, ilabel, olabel, weight, dst).  Arc ids are the arcs'
 * positions after a stable sort by src.  ilabel 0 is an epsilon arc (consumes
 * no frame); ilabel i >= 1 consumes one frame and reads column col(i) =
 * ilabel_to_col[i] of the log-likelihood row (default i - 1: "transition-id 1
 * is blank" under a trivial transition model; otherwise the table
 * CtcTransitionModel::TransitionIdToPdf gives).  olabel 0 emits nothing.
 *
 * The graph functions return 0 or non-zero with kctc_last_error(); they need
 * no GPU.  The device image of a graph is made (one allocation, one blocking
 * copy) by the first decode on a device and freed by kctc_graph_destroy. */
typedef struct kctcGraphImpl *kctcGraph_t;

/* Builds a graph from host arrays: final_costs [num_states], the five arc
 * arrays [num_arcs] in any order.  ilabel_to_col: nullable, else num_ilabels
 * ints indexed by ilabel (entry 0 unused).  Refuses, before anything else
 * happens: a state or start index out of range, a negative label, an ilabel
 * >= num_ilabels, a non-finite arc weight, a final cost that is NaN or -inf, a
 * negative column, an epsilon cycle.  Computes eps_depth, the number of arcs
 * on the longest epsilon path: the bound of the search's closure loop. */
int kctc_graph_create(kctcGraph_t *graph, int num_states, int start, const float *final_costs, long num_arcs,
                      const int *src, const int *ilabel, const int *olabel, const float *weight, const int *dst,
                      const int *ilabel_to_col, int num_ilabels);

/* OpenFst text form (what fstprint writes without symbol tables): arc lines
 * "src dst ilabel olabel [weight]", final lines "state [weight]", a missing
 * weight is 0, the start state is the source of the first line, labels are
 * integers.  num_states = the highest state named + 1.  Binary .fst files are
 * not read.  kctc_graph_write_text writes the start state's lines first and
 * weights with 9 digits, so that reading the file back gives the same graph
 * with the same arc ids. */
int kctc_graph_read_text(kctcGraph_t *graph, const char *path, const int *ilabel_to_col, int num_ilabels);
int kctc_graph_write_text(kctcGraph_t graph, const char *path);

/* Outputs (nullable): states, arcs, eps_depth, the highest ilabel and the
 * highest column an emitting arc reads (-1: no emitting arc). */
int kctc_graph_info(kctcGraph_t graph, int *num_states, long *num_arcs, int *eps_depth, int *max_ilabel,
                    int *max_col);

/* The graph as it is stored (nullable outputs): start, final_costs
 * [num_states] and the arcs in arc-id order, [num_arcs] each. */
int kctc_graph_get(kctcGraph_t graph, int *start, float *final_costs, int *src, int *ilabel, int *olabel,
                   float *weight, int *dst);

int kctc_graph_destroy(kctcGraph_t graph);

/* Viterbi token passing, one utterance per workgroup.  Per utterance, with
 * ac(t, i) = -acoustic_scale * loglikes[t][n][col(i)]:
 *   a token set holds at most one token per state; a candidate replaces a
 *   token only if (cost, arc id) is lexicographically smaller (the start
 *   token: arc id -1);
 *   closure(Q) relaxes every epsilon arc to the fixed point, nothing pruned;
 *   Q_0 = closure({start: 0});
 *   frame t: best = min cost of Q_t; E_t = the first min(max_active, count)
 *   tokens of {cost <= best + beam} in (cost, state id) order (exact);
 *   Q_{t+1} = closure(emit(E_t)), every emitting arc of every token of E_t
 *   relaxed with cost + weight + ac(t, ilabel), nothing pruned;
 *   after T frames: the token of Q_T with the smallest cost + final cost over
 *   final states (status 1); if none is final the token of smallest cost
 *   (status 0); Q_T empty: status -1; more than pool_tokens back-pointer
 *   records (one per token of every Q_t, t = 0..T): status -2.  A negative
 *   status gives words_len 0, ali -1, score +inf and leaves the other
 *   utterances alone.  T = 0 evaluates Q_0.
 * Costs are fp32 relative to a per-utterance fp64 offset that takes each
 * frame's best; the selection compares those fp32 values.  A candidate whose
 * cost is NaN or infinite starts no token.
 *
 * loglikes [maxT][N][num_columns] floats, device, time-major, maxT =
 * max(input_lengths); rows t >= input_lengths[n] are never read.
 * input_lengths: host, >= 0.  beam > 0 (+inf allowed), 1 <= max_active <= 2^20,
 * 1 <= pool_tokens < 2^31 - 2.  Outputs, device:
 *   words     [N][maxT + W] ints, W = (maxT + 1) * eps_depth: the non-zero
 *             olabels of the path in order, then -1 (a path has T emitting arcs
 *             and at most eps_depth epsilon arcs before, between and behind them)
 *   words_len [N];  ali [maxT][N]: the ilabel of frame t's arc, -1 for t >= T
 *   scores    [N] doubles: graph + acoustic + final cost;  status [N]
 * workspace: kctc_wfst_decode_workspace_size bytes =
 *   N * (52 * num_states + 4 * (maxT + 2) + 8 * pool_tokens) + at most
 *   4096 + 2592 * N of descriptors and alignment.
 * Returns 0, or 2 (the value of CTC_STATUS_INVALID_VALUE) with nothing
 * enqueued for a null pointer, a negative length, a column >= num_columns, a
 * parameter out of range; 1 / 3 for a failed copy / launch; 4 for an exception
 * (the graph's device image could not be made: kctc_last_error()).  Asynchronous: it
 * never synchronises the stream and allocates nothing, except that the first
 * decode of a graph on a device makes the graph's device image.  Two calls on
 * the same inputs give identical bytes in all five outputs. */
int kctc_wfst_decode_workspace_size(kctcGraph_t graph, const int *input_lengths, int minibatch, int max_active,
                                    long pool_tokens, size_t *size_bytes);
int kctc_wfst_decode_async(kctcGraph_t graph, const float *loglikes, const int *input_lengths, int num_columns,
                           int minibatch, float acoustic_scale, float beam, int max_active, long pool_tokens,
                           int *words_dev, int *words_len_dev, int *ali_dev, double *scores_dev, int *status_dev,
                           void *workspace, struct ihipStream_t *stream);

/* What the last kctc_wfst_decode_async on `workspace` did, per utterance
 * (host arrays of `minibatch` longs): expanded = the sum over its frames of
 * |E_t|, held = the sum over t = 0..T of |Q_t| (the back-pointer records it
 * used).  Copies from the workspace on `stream` and synchronises it. */
int kctc_wfst_decode_counts(const void *workspace, int minibatch, struct ihipStream_t *stream, long *expanded,
                            long *held);

/* nnet2-ctc-latgen-faster's best path for a batch.  feats_dev, T_max, N,
 * num_frames as for kctc_nnet_propagate_seq (N <= 64): the variable-length
 * forward, a softmax if the network does not end in one, then on the device
 * (log(max(p, 1e-10)) - log prior) * prob_scale with the model's priors (none
 * if the model has none) and all frames kept, then kctc_wfst_decode_async on
 * the network's stream with acoustic_scale.  prob_scale is
 * CtcDecodableAmNnet's scale of the log-likelihoods, acoustic_scale the
 * decoder's own; the reference uses one of them and leaves the other at 1.
 * pool_tokens <= 0: (T_max + 1) * min(num_states, 4 * max_active + 4096).  Outputs,
 * host: words_host [N][words_stride] (the first min(words_len, words_stride)
 * words of each path, then -1), words_len_host [N], ali_host [T_max][N] (-1
 * for t >= num_frames[n]), scores_host [N], status_host [N]. */
int kctc_nnet_decode_graph(kctcNnet_t nnet, kctcGraph_t graph, const float *feats_dev, int T_max, int N,
                           const int *num_frames, float prob_scale, float acoustic_scale, float beam, int max_active,
                           long pool_tokens, int *words_host, int words_stride, int *words_len_host, int *ali_host,
                           double *scores_host, int *status_host);

/* Decodes every example of an egs archive (read as kctc_nnet_decode_egs reads
 * it) and writes, per example key, the words as a Kaldi Int32Vector to a binary
 * "ark:" (Kaldi's words.tra as a table) and, if ali_wspecifier is not null,
 * the per-frame ilabels to a second one.  Utterances with a negative status
 * are counted and not written.  Outputs (nullable): utterances decoded
 * (status >= 0), how many of them reached a final state, utterances that
 * failed, the sum of the decoded utterances' scores and of their frames. */
int kctc_nnet_decode_graph_egs(kctcNnet_t nnet, kctcGraph_t graph, const char *egs_rspecifier,
                               const char *words_wspecifier, const char *ali_wspecifier, int minibatch_size,
                               float prob_scale, float acoustic_scale, float beam, int max_active, long pool_tokens,
                               long *num_done, long *num_final, long *num_failed, double *tot_score,
                               long *tot_frames);

#ifdef __cplusplus
}
#endif
#endif /* KALDI_CTC_AMD_KALDI_CTC_DECODE_H_ */
