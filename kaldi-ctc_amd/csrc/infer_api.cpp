// infer_api.cpp -- C ABI of include/kaldi_ctc_decode.h and the forward-only
// entry points of kaldi_ctc_train.h: propagate, the CTC decodable (one
// utterance and batched), posterior sums, priors, compute-prob, and the CTC
// forced alignment, prefix beam search and graph search of a batch or an egs
// archive.
#include "kaldi_ctc_decode.h"

#include <algorithm>
#include <fstream>
#include <string>
#include <vector>

#include "ctc.h"
#include "decodable.h"
#include "elementwise.h"
#include "kaldi_io.h"
#include "nnet_handle.h"
#include "seq_align.h"
#include "wfst_decode.h"

using kctc::nnet2::CuDevice;

// the model's priors on the device (nullptr: none), uploaded again only when they change
static const float *device_priors(kctcNnet_t n, int A) {
  if (n->priors.empty()) return nullptr;
  KCTC_REQUIRE((int)n->priors.size() == A, "priors dimension != network output dimension");
  if (n->dec_priors_host != n->priors) {
    n->dec_priors.ensure(sizeof(float) * A);
    KCTC_HIP_CHECK(hipMemcpyAsync(n->dec_priors.p, n->priors.data(), sizeof(float) * A, hipMemcpyHostToDevice,
                                  n->stream));
    KCTC_HIP_CHECK(hipStreamSynchronize(n->stream));  // the source is the host vector
    n->dec_priors_host = n->priors;
  }
  return n->dec_priors.f();
}

// kctc_nnet_profile of the forward-only entry points: their spans are complete
// after the stream synchronisation (a training step in flight collects its own)
static void collect_profile(kctcNnet_t n) {
  if (n->trainer.Pending() == 0 && n->evaluator.Pending() == 0) CuDevice::Instantiate().Collect();
}

// device-to-device copy of a forward's output into the caller's buffer
static void copy_out(kctcNnet_t n, const kctc::nnet2::CuMatrixBase &o, float *out_dev, long len, const char *what) {
  KCTC_REQUIRE(len == o.NumRows() * (long)o.NumCols(), what);
  KCTC_HIP_CHECK(hipMemcpyAsync(out_dev, o.Data(), sizeof(float) * len, hipMemcpyDeviceToDevice, n->stream));
  KCTC_HIP_CHECK(hipStreamSynchronize(n->stream));
}

// Reads the egs archive and calls fn(batch) for every batch_size examples and
// for the rest; returns the number of examples.
template <typename F>
static long for_each_batch(const char *rspecifier, size_t batch_size, F fn) {
  kctc::egs::ArchiveReader reader(rspecifier);
  std::vector<kctc::egs::Example> batch;
  long ne = 0;
  kctc::egs::Example eg;
  while (reader.Next(&eg)) {
    if (batch.size() == batch_size) {
      fn(batch);
      batch.clear();
    }
    batch.push_back(std::move(eg));
    eg = kctc::egs::Example();
    ne++;
  }
  if (!batch.empty()) fn(batch);
  return ne;
}

// file name of a binary "ark:" wspecifier (a bare file name passes)
static std::string ark_path(const char *wspecifier) {
  std::string path = wspecifier;
  const auto colon = path.find(':');
  if (colon != std::string::npos) {
    KCTC_REQUIRE(path.compare(0, 3, "ark") == 0, "only ark: specifiers are supported");
    path = path.substr(colon + 1);
  }
  return path;
}

// Kaldi table entry: "<key> " then the binary marker and the Int32Vector
static void write_int_vector_entry(std::ostream &os, const std::string &key, const std::vector<int32_t> &v) {
  os << key << ' ';
  os.put('\0');
  os.put('B');
  kctc::kio::WriteIntVector(os, true, v);
}

// The un-normalised activations of the last forward: a final SoftmaxComponent
// (the recipe's final.mdl) only shifts every row's log by a constant, which
// the CTC kernels' own normaliser removes, so they run on its input.
static const kctc::nnet2::CuMatrixBase &unnormalised_output(kctcNnet_t n) {
  const int C = n->nnet.NumComponents();
  const bool softmax = dynamic_cast<const kctc::nnet2::SoftmaxComponent *>(&n->nnet.GetComponent(C - 1)) != nullptr;
  return n->evaluator.InputOf(softmax ? C - 1 : C);
}

// kctc_nnet_decode on a formatted input: variable-length forward, then the
// prefix beam search on the network's stream; hyp_host is [N][T_max]
static void decode_batch(kctcNnet_t n, const float *feats_dev, int T_max, int N, const int *num_frames, int beam,
                         int symbols, int *hyp_host, int *hyp_len_host, double *scores_host) {
  KCTC_REQUIRE(N >= 1 && N <= kctc::kSeqMaxN, "kctc_nnet_decode: N outside [1, 64]");
  n->evaluator.ForwardSeq(feats_dev, T_max, N, num_frames);
  const auto &o = unnormalised_output(n);
  const int A = o.NumCols();
  int maxT = 0;
  for (int u = 0; u < N; u++) maxT = std::max(maxT, num_frames[u]);
  size_t ws = 0;
  ctcStatus_t st = mictc_get_beam_workspace_size(num_frames, A, N, beam, &ws);
  if (st != CTC_STATUS_SUCCESS)
    throw std::invalid_argument(std::string("mictc_get_beam_workspace_size: ") + ctcGetStatusString(st));
  n->beam_ws.ensure(ws);
  n->beam_hyp.ensure(sizeof(int) * (size_t)maxT * N);
  n->beam_len.ensure(sizeof(int) * N);
  n->beam_scores.ensure(sizeof(double) * N);
  st = mictc_ctc_beam_search_async(o.Data(), num_frames, A, N, beam, symbols, static_cast<int *>(n->beam_hyp.p),
                                   static_cast<int *>(n->beam_len.p), static_cast<double *>(n->beam_scores.p),
                                   n->beam_ws.p, reinterpret_cast<ctcStream_t>(n->stream), 0);
  if (st != CTC_STATUS_SUCCESS)
    throw std::invalid_argument(std::string("mictc_ctc_beam_search_async: ") + ctcGetStatusString(st));
  // the search fills max(num_frames) columns; T_max may be longer
  std::fill(hyp_host, hyp_host + (size_t)T_max * N, -1);
  if (maxT > 0)
    KCTC_HIP_CHECK(hipMemcpy2DAsync(hyp_host, sizeof(int) * T_max, n->beam_hyp.p, sizeof(int) * maxT,
                                    sizeof(int) * maxT, N, hipMemcpyDeviceToHost, n->stream));
  KCTC_HIP_CHECK(hipMemcpyAsync(hyp_len_host, n->beam_len.p, sizeof(int) * N, hipMemcpyDeviceToHost, n->stream));
  KCTC_HIP_CHECK(hipMemcpyAsync(scores_host, n->beam_scores.p, sizeof(double) * N, hipMemcpyDeviceToHost, n->stream));
  KCTC_HIP_CHECK(hipStreamSynchronize(n->stream));
}

extern "C" {

int kctc_nnet_decode(kctcNnet_t n, const float *feats_dev, int T_max, int N, const int *num_frames, int beam,
                     int symbols, int *hyp_host, int *hyp_len_host, double *scores_host) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n && feats_dev && num_frames && hyp_host && hyp_len_host && scores_host,
                 "kctc_nnet_decode: null argument");
    n->activate();
    decode_batch(n, feats_dev, T_max, N, num_frames, beam, symbols, hyp_host, hyp_len_host, scores_host);
    collect_profile(n);
  });
}

int kctc_nnet_decode_egs(kctcNnet_t n, const char *egs_rspecifier, const char *hyp_wspecifier, int minibatch_size,
                         int beam, int symbols, long *num_utts, long *num_labels, long *edit_distance) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n && egs_rspecifier && hyp_wspecifier, "kctc_nnet_decode_egs: null argument");
    KCTC_REQUIRE(minibatch_size >= 1 && minibatch_size <= kctc::kSeqMaxN,
                 "kctc_nnet_decode_egs: minibatch_size outside [1, 64]");
    const std::string path = ark_path(hyp_wspecifier);
    n->activate();
    std::ofstream os(path, std::ios::binary | std::ios::trunc);
    if (!os) throw std::runtime_error("cannot write hypothesis archive " + path);
    long utts = 0, labels = 0, errs = 0;
    std::vector<int> hyp, hyp_len;
    std::vector<double> scores;
    for_each_batch(egs_rspecifier, minibatch_size, [&](std::vector<kctc::egs::Example> &batch) {
      // every example from its own start offset, pad_input = false (as kctc_nnet_sum_posteriors)
      std::unique_ptr<kctc::egs::Minibatch> mb =
          kctc::egs::pack_minibatch(batch, n->nnet.LeftContext(), n->nnet.RightContext(), true);
      n->check_input_dim(*mb);
      kctc::SeqLens lens;
      if (!kctc::seq_lens(mb->num_frames.data(), mb->T_max, mb->N, &lens))
        throw std::invalid_argument("an example is shorter than the network's context");
      n->stage_minibatch(*mb);
      const int N = mb->N, T_max = mb->T_max;
      hyp.resize((size_t)T_max * N);
      hyp_len.resize(N);
      scores.resize(N);
      decode_batch(n, n->egs_feats.f(), T_max, N, mb->num_frames.data(), beam, symbols, hyp.data(), hyp_len.data(),
                   scores.data());
      size_t lab_off = 0;
      for (int u = 0; u < N; u++) {
        const int *h = hyp.data() + (size_t)u * T_max;
        const int L = mb->label_lengths[u];
        write_int_vector_entry(os, mb->keys[u], std::vector<int32_t>(h, h + hyp_len[u]));
        // LevenshteinEditDistance to the example's own labels, as compute_prob's accuracy counts it
        errs += kctc::nnet2::levenshtein(mb->labels.data() + lab_off, L, h, hyp_len[u]);
        lab_off += L;
        labels += L;
        utts++;
      }
    });
    os.flush();
    if (!os) throw std::runtime_error("error writing hypothesis archive " + path);
    collect_profile(n);
    if (num_utts) *num_utts = utts;
    if (num_labels) *num_labels = labels;
    if (edit_distance) *edit_distance = errs;
  });
}

}  // extern "C"

// kctc_nnet_decode_graph on a formatted input: variable-length forward, the
// decodable rows of every utterance (all frames kept, utterance after
// utterance), then the graph search on the network's stream
struct GraphDecodeOpts {
  float prob_scale, acoustic_scale, beam;
  int max_active;
  long pool_tokens;
};
static void decode_graph_batch(kctcNnet_t n, kctcGraph_t g, const float *feats_dev, int T_max, int N,
                               const int *num_frames, const GraphDecodeOpts &opt, int *words_host, int words_stride,
                               int *words_len_host, int *ali_host, double *scores_host, int *status_host) {
  KCTC_REQUIRE(N >= 1 && N <= kctc::kSeqMaxN, "kctc_nnet_decode_graph: N outside [1, 64]");
  KCTC_REQUIRE(words_stride >= 1, "kctc_nnet_decode_graph: words_stride < 1");
  kctc::SeqLens lens;
  KCTC_REQUIRE(kctc::seq_lens(num_frames, T_max, N, &lens), "kctc_nnet_decode_graph: num_frames outside [1, T_max]");
  const auto &o = n->evaluator.ForwardSeq(feats_dev, T_max, N, num_frames);
  const int A = o.NumCols(), C = n->nnet.NumComponents();
  const float *probs = o.Data();
  if (!dynamic_cast<const kctc::nnet2::SoftmaxComponent *>(&n->nnet.GetComponent(C - 1))) {
    n->wfst_probs.ensure(sizeof(float) * (size_t)T_max * N * A);
    kctc::softmax_rows(n->stream, o.Data(), (long)T_max * N, A, n->wfst_probs.f());
    probs = n->wfst_probs.f();
  }
  const float *pd = device_priors(n, A);
  long total = 0;
  int maxT = 0;
  std::vector<long long> ll_off((size_t)N), ll_stride((size_t)N, A);
  for (int u = 0; u < N; u++) {
    ll_off[u] = total * A;
    total += num_frames[u];
    maxT = std::max(maxT, num_frames[u]);
  }
  n->dec_out.ensure(sizeof(float) * (size_t)total * A);
  n->dec_scratch.ensure(kctc::seq_decodable_scratch_bytes(T_max, N));
  n->dec_kept.ensure(sizeof(int) * kctc::kSeqMaxN);
  // blank_threshold 1: no frame is dropped, utterance u's rows start at row sum(num_frames[< u])
  kctc::seq_decodable(n->stream, probs, T_max, N, A, lens, pd, opt.prob_scale, 1.0f, 1.0e-10f, n->dec_out.f(),
                      n->dec_scratch.p, static_cast<int *>(n->dec_kept.p));
  int S = 0, depth = 0;
  if (kctc_graph_info(g, &S, nullptr, &depth, nullptr, nullptr)) throw std::runtime_error(kctc_last_error());
  const long pool = opt.pool_tokens > 0 ? opt.pool_tokens
                                        : ((long)T_max + 1) * std::min<long>(S, 4l * std::max(opt.max_active, 1) + 4096);
  const size_t ws = kctc::wfst::decode_workspace_bytes(g, num_frames, N, opt.max_active, pool);
  KCTC_REQUIRE(ws > 0, "kctc_nnet_decode_graph: max_active or pool_tokens out of range");
  const size_t row = (size_t)maxT + (size_t)kctc::wfst::words_slack(depth, maxT);
  n->wfst_ws.ensure(ws);
  n->wfst_words.ensure(sizeof(int) * row * N);
  n->wfst_len.ensure(sizeof(int) * N);
  n->wfst_ali.ensure(sizeof(int) * (size_t)maxT * N);
  n->wfst_scores.ensure(sizeof(double) * N);
  n->wfst_status.ensure(sizeof(int) * N);
  const int st = kctc::wfst::decode_strided(
      g, n->dec_out.f(), num_frames, ll_off.data(), ll_stride.data(), A, N, opt.acoustic_scale, opt.beam,
      opt.max_active, pool, static_cast<int *>(n->wfst_words.p), static_cast<int *>(n->wfst_len.p),
      static_cast<int *>(n->wfst_ali.p), static_cast<double *>(n->wfst_scores.p), static_cast<int *>(n->wfst_status.p),
      n->wfst_ws.p, n->stream);
  if (st == 2)
    throw std::invalid_argument("kctc_wfst_decode_async: invalid value (beam, max_active, pool_tokens, or the graph "
                                "reads a column the network does not output)");
  if (st) throw std::runtime_error("kctc_wfst_decode_async failed");
  std::fill(words_host, words_host + (size_t)words_stride * N, -1);
  std::fill(ali_host, ali_host + (size_t)T_max * N, -1);
  const size_t wcopy = std::min<size_t>(row, (size_t)words_stride);
  KCTC_HIP_CHECK(hipMemcpy2DAsync(words_host, sizeof(int) * words_stride, n->wfst_words.p, sizeof(int) * row,
                                  sizeof(int) * wcopy, N, hipMemcpyDeviceToHost, n->stream));
  KCTC_HIP_CHECK(hipMemcpyAsync(ali_host, n->wfst_ali.p, sizeof(int) * (size_t)maxT * N, hipMemcpyDeviceToHost,
                                n->stream));
  KCTC_HIP_CHECK(hipMemcpyAsync(words_len_host, n->wfst_len.p, sizeof(int) * N, hipMemcpyDeviceToHost, n->stream));
  KCTC_HIP_CHECK(hipMemcpyAsync(scores_host, n->wfst_scores.p, sizeof(double) * N, hipMemcpyDeviceToHost, n->stream));
  KCTC_HIP_CHECK(hipMemcpyAsync(status_host, n->wfst_status.p, sizeof(int) * N, hipMemcpyDeviceToHost, n->stream));
  KCTC_HIP_CHECK(hipStreamSynchronize(n->stream));
}

extern "C" {

int kctc_nnet_decode_graph(kctcNnet_t n, kctcGraph_t g, const float *feats_dev, int T_max, int N,
                           const int *num_frames, float prob_scale, float acoustic_scale, float beam, int max_active,
                           long pool_tokens, int *words_host, int words_stride, int *words_len_host, int *ali_host,
                           double *scores_host, int *status_host) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n && g && feats_dev && num_frames && words_host && words_len_host && ali_host && scores_host &&
                     status_host,
                 "kctc_nnet_decode_graph: null argument");
    n->activate();
    decode_graph_batch(n, g, feats_dev, T_max, N, num_frames,
                       GraphDecodeOpts{prob_scale, acoustic_scale, beam, max_active, pool_tokens}, words_host,
                       words_stride, words_len_host, ali_host, scores_host, status_host);
    collect_profile(n);
  });
}

int kctc_nnet_decode_graph_egs(kctcNnet_t n, kctcGraph_t g, const char *egs_rspecifier, const char *words_wspecifier,
                               const char *ali_wspecifier, int minibatch_size, float prob_scale, float acoustic_scale,
                               float beam, int max_active, long pool_tokens, long *num_done, long *num_final,
                               long *num_failed, double *tot_score, long *tot_frames) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n && g && egs_rspecifier && words_wspecifier, "kctc_nnet_decode_graph_egs: null argument");
    KCTC_REQUIRE(minibatch_size >= 1 && minibatch_size <= kctc::kSeqMaxN,
                 "kctc_nnet_decode_graph_egs: minibatch_size outside [1, 64]");
    const std::string wpath = ark_path(words_wspecifier), apath = ali_wspecifier ? ark_path(ali_wspecifier) : "";
    n->activate();
    std::ofstream wos(wpath, std::ios::binary | std::ios::trunc), aos;
    if (!wos) throw std::runtime_error("cannot write word archive " + wpath);
    if (ali_wspecifier) {
      aos.open(apath, std::ios::binary | std::ios::trunc);
      if (!aos) throw std::runtime_error("cannot write alignment archive " + apath);
    }
    int depth = 0;
    if (kctc_graph_info(g, nullptr, nullptr, &depth, nullptr, nullptr)) throw std::runtime_error(kctc_last_error());
    long done = 0, fin = 0, failed = 0, frames = 0;
    double score = 0.0;
    std::vector<int> words, words_len, ali, status;
    std::vector<double> scores;
    const GraphDecodeOpts opt{prob_scale, acoustic_scale, beam, max_active, pool_tokens};
    for_each_batch(egs_rspecifier, minibatch_size, [&](std::vector<kctc::egs::Example> &batch) {
      // every example from its own start offset, pad_input = false (as kctc_nnet_sum_posteriors)
      std::unique_ptr<kctc::egs::Minibatch> mb =
          kctc::egs::pack_minibatch(batch, n->nnet.LeftContext(), n->nnet.RightContext(), true);
      n->check_input_dim(*mb);
      kctc::SeqLens lens;
      if (!kctc::seq_lens(mb->num_frames.data(), mb->T_max, mb->N, &lens))
        throw std::invalid_argument("an example is shorter than the network's context");
      n->stage_minibatch(*mb);
      const int N = mb->N, T_max = mb->T_max;
      const size_t row = (size_t)T_max + (size_t)kctc::wfst::words_slack(depth, T_max);
      KCTC_REQUIRE(row < (size_t)INT_MAX, "kctc_nnet_decode_graph_egs: the word rows are too long");
      words.resize(row * N);
      words_len.resize(N);
      ali.resize((size_t)T_max * N);
      scores.resize(N);
      status.resize(N);
      decode_graph_batch(n, g, n->egs_feats.f(), T_max, N, mb->num_frames.data(), opt, words.data(), (int)row,
                         words_len.data(), ali.data(), scores.data(), status.data());
      for (int u = 0; u < N; u++) {
        if (status[u] < 0) {
          failed++;
          continue;
        }
        const int *w = words.data() + row * u;
        write_int_vector_entry(wos, mb->keys[u], std::vector<int32_t>(w, w + words_len[u]));
        const int T = mb->num_frames[u];
        if (ali_wspecifier) {
          std::vector<int32_t> v((size_t)T);
          for (int t = 0; t < T; t++) v[t] = ali[(size_t)t * N + u];
          write_int_vector_entry(aos, mb->keys[u], v);
        }
        done++;
        fin += status[u] == 1 ? 1 : 0;
        score += scores[u];
        frames += T;
      }
    });
    wos.flush();
    if (!wos) throw std::runtime_error("error writing word archive " + wpath);
    if (ali_wspecifier) {
      aos.flush();
      if (!aos) throw std::runtime_error("error writing alignment archive " + apath);
    }
    collect_profile(n);
    if (num_done) *num_done = done;
    if (num_final) *num_final = fin;
    if (num_failed) *num_failed = failed;
    if (tot_score) *tot_score = score;
    if (tot_frames) *tot_frames = frames;
  });
}

}  // extern "C"

// kctc_nnet_align on a formatted input: variable-length forward, then the
// alignment of the un-normalised activations on the network's stream
static void align_batch(kctcNnet_t n, const float *feats_dev, int T_max, int N, const int *num_frames,
                        const int *flat_labels, const int *label_lengths, int *ali_host, double *scores_host) {
  KCTC_REQUIRE(N >= 1 && N <= kctc::kSeqMaxN, "kctc_nnet_align: N outside [1, 64]");
  n->evaluator.ForwardSeq(feats_dev, T_max, N, num_frames);
  const auto &o = unnormalised_output(n);
  const int A = o.NumCols();
  const size_t rows = (size_t)T_max * N;
  size_t ws = 0;
  // CTC input lengths: NumFrames - ignore_frames, 0 ignored here as in the updater
  ctcStatus_t st = mictc_get_align_workspace_size(label_lengths, num_frames, A, N, &ws);
  if (st != CTC_STATUS_SUCCESS)
    throw std::invalid_argument(std::string("mictc_get_align_workspace_size: ") + ctcGetStatusString(st));
  n->ali_ws.ensure(ws);
  n->ali_ids.ensure(sizeof(int) * rows);
  n->ali_scores.ensure(sizeof(double) * N);
  int *ids = static_cast<int *>(n->ali_ids.p);
  // the alignment fills rows below max(num_frames); T_max may be longer
  KCTC_HIP_CHECK(hipMemsetAsync(ids, 0xFF, sizeof(int) * rows, n->stream));
  st = mictc_ctc_align_async(o.Data(), flat_labels, label_lengths, num_frames, A, N, ids,
                             static_cast<double *>(n->ali_scores.p), n->ali_ws.p,
                             reinterpret_cast<ctcStream_t>(n->stream), 0);
  if (st != CTC_STATUS_SUCCESS)
    throw std::invalid_argument(std::string("mictc_ctc_align_async: ") + ctcGetStatusString(st));
  KCTC_HIP_CHECK(hipMemcpyAsync(ali_host, ids, sizeof(int) * rows, hipMemcpyDeviceToHost, n->stream));
  KCTC_HIP_CHECK(hipMemcpyAsync(scores_host, n->ali_scores.p, sizeof(double) * N, hipMemcpyDeviceToHost, n->stream));
  KCTC_HIP_CHECK(hipStreamSynchronize(n->stream));
}

extern "C" {

int kctc_nnet_align(kctcNnet_t n, const float *feats_dev, int T_max, int N, const int *num_frames,
                    const int *flat_labels, const int *label_lengths, int *ali_host, double *scores_host) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n && feats_dev && num_frames && flat_labels && label_lengths && ali_host && scores_host,
                 "kctc_nnet_align: null argument");
    n->activate();
    align_batch(n, feats_dev, T_max, N, num_frames, flat_labels, label_lengths, ali_host, scores_host);
    collect_profile(n);
  });
}

int kctc_nnet_align_egs(kctcNnet_t n, const char *egs_rspecifier, const char *ali_wspecifier, int minibatch_size,
                        long *num_done, long *num_infeasible, double *tot_score, long *tot_frames) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n && egs_rspecifier && ali_wspecifier, "kctc_nnet_align_egs: null argument");
    KCTC_REQUIRE(minibatch_size >= 1 && minibatch_size <= kctc::kSeqMaxN,
                 "kctc_nnet_align_egs: minibatch_size outside [1, 64]");
    const std::string path = ark_path(ali_wspecifier);
    n->activate();
    std::ofstream os(path, std::ios::binary | std::ios::trunc);
    if (!os) throw std::runtime_error("cannot write alignment archive " + path);
    long done = 0, infeasible = 0, frames = 0;
    double score = 0.0;
    std::vector<int> ids;
    std::vector<double> scores;
    for_each_batch(egs_rspecifier, minibatch_size, [&](std::vector<kctc::egs::Example> &batch) {
      // every example from its own start offset, pad_input = false (as kctc_nnet_sum_posteriors)
      std::unique_ptr<kctc::egs::Minibatch> mb =
          kctc::egs::pack_minibatch(batch, n->nnet.LeftContext(), n->nnet.RightContext(), true);
      n->check_input_dim(*mb);
      kctc::SeqLens lens;
      if (!kctc::seq_lens(mb->num_frames.data(), mb->T_max, mb->N, &lens))
        throw std::invalid_argument("an example is shorter than the network's context");
      n->stage_minibatch(*mb);
      const int N = mb->N, T_max = mb->T_max;
      ids.resize((size_t)T_max * N);
      scores.resize(N);
      const int none = 0;  // a batch without labels still passes a valid pointer
      align_batch(n, n->egs_feats.f(), T_max, N, mb->num_frames.data(), mb->labels.empty() ? &none : mb->labels.data(),
                  mb->label_lengths.data(), ids.data(), scores.data());
      for (int u = 0; u < N; u++) {
        if (ids[u] < 0) {  // frame 0 of an infeasible utterance is -1
          infeasible++;
          continue;
        }
        const int T = mb->num_frames[u];
        std::vector<int32_t> v((size_t)T);
        for (int t = 0; t < T; t++) v[t] = ids[(size_t)t * N + u];
        write_int_vector_entry(os, mb->keys[u], v);
        done++;
        frames += T;
        score += scores[u];
      }
    });
    os.flush();
    if (!os) throw std::runtime_error("error writing alignment archive " + path);
    collect_profile(n);
    if (num_done) *num_done = done;
    if (num_infeasible) *num_infeasible = infeasible;
    if (tot_score) *tot_score = score;
    if (tot_frames) *tot_frames = frames;
  });
}

size_t kctc_ctc_decodable_scratch_bytes(int T) { return kctc::ctc_decodable_scratch_bytes(T > 0 ? T : 1) + 256; }

int kctc_softmax_rows(struct ihipStream_t *stream, const float *in, long rows, int cols, float *out) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(in && out && rows >= 0 && cols > 0, "kctc_softmax_rows: bad argument");
    kctc::softmax_rows(stream, in, rows, cols, out);
    KCTC_HIP_CHECK(hipGetLastError());
  });
}

int kctc_ctc_decodable(struct ihipStream_t *stream, const float *probs, int T, int A, const float *priors,
                       float prob_scale, float blank_threshold, float floor_value, float *out, void *scratch,
                       int *num_kept) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(probs && out && scratch && num_kept && T > 0 && A > 0, "kctc_ctc_decodable: bad argument");
    int *kept_dev = reinterpret_cast<int *>(static_cast<char *>(scratch) + kctc::ctc_decodable_scratch_bytes(T));
    kctc::ctc_decodable(stream, probs, T, A, priors, prob_scale, blank_threshold, floor_value, out, scratch,
                        kept_dev);
    KCTC_HIP_CHECK(hipGetLastError());
    KCTC_HIP_CHECK(hipMemcpyAsync(num_kept, kept_dev, sizeof(int), hipMemcpyDeviceToHost, stream));
    KCTC_HIP_CHECK(hipStreamSynchronize(stream));
  });
}

int kctc_nnet_propagate(kctcNnet_t n, const float *feats_dev, int T_max, int N, float *out_dev, long len) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n && feats_dev && out_dev, "kctc_nnet_propagate: null argument");
    n->activate();
    copy_out(n, n->evaluator.Forward(feats_dev, T_max, N), out_dev, len,
             "kctc_nnet_propagate: len != T_max*N*output_dim");
  });
}

int kctc_am_nnet_decodable(kctcNnet_t n, const float *feats_dev, int T, float prob_scale, float blank_threshold,
                           float *out_host, int *num_rows) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n && feats_dev && out_host && num_rows && T > 0, "kctc_am_nnet_decodable: bad argument");
    n->activate();
    // NnetComputation(nnet, feats, pad_input = true) (ctc-decodable-am-nnet.cc:28-52,
    // nnet-compute.cc:64-90): T output frames from the T feature rows, the
    // first / last frame repeated LeftContext / RightContext times; a spliced
    // network reads num_splice rows per output frame (FormatNnetInput layout)
    const float *in = feats_dev;
    const int ns = n->nnet.NumSplice();
    if (ns > 1) {
      n->dec_input.ensure(sizeof(float) * (size_t)T * ns * n->nnet.InputDim());
      kctc::pad_splice_input(n->stream, feats_dev, T, n->nnet.InputDim(), n->nnet.LeftContext(), ns,
                             n->dec_input.f());
      in = n->dec_input.f();
    }
    const auto &o = n->evaluator.Forward(in, T, 1);
    const int A = o.NumCols();
    auto &out = n->dec_out, &scratch = n->dec_scratch;
    const float *pd = device_priors(n, A);
    out.ensure(sizeof(float) * (size_t)T * A);
    scratch.ensure(kctc_ctc_decodable_scratch_bytes(T));
    int kept = 0;
    const int st = kctc_ctc_decodable(n->stream, o.Data(), T, A, pd, prob_scale, blank_threshold, 1.0e-10f, out.f(),
                                      scratch.p, &kept);
    if (st) throw std::runtime_error(kctc_last_error());
    KCTC_HIP_CHECK(hipStreamSynchronize(n->stream));
    KCTC_HIP_CHECK(hipMemcpy(out_host, out.p, sizeof(float) * (size_t)kept * A, hipMemcpyDeviceToHost));
    *num_rows = kept;
  });
}

int kctc_nnet_propagate_seq(kctcNnet_t n, const float *feats_dev, int T_max, int N, const int *num_frames,
                            float *out_dev, long len) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n && feats_dev && out_dev && num_frames, "kctc_nnet_propagate_seq: null argument");
    n->activate();
    copy_out(n, n->evaluator.ForwardSeq(feats_dev, T_max, N, num_frames), out_dev, len,
             "kctc_nnet_propagate_seq: len != T_max*N*output_dim");
    collect_profile(n);
  });
}

int kctc_am_nnet_decodable_batch(kctcNnet_t n, const float *feats_dev, int T_max, int N, const int *num_frames,
                                 float prob_scale, float blank_threshold, float *out_host, int *rows) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n && feats_dev && num_frames && out_host && rows && T_max > 0 && N > 0,
                 "kctc_am_nnet_decodable_batch: bad argument");
    long total = 0;
    for (int u = 0; u < N; u++) {
      KCTC_REQUIRE(num_frames[u] >= 1 && num_frames[u] <= T_max,
                   "kctc_am_nnet_decodable_batch: num_frames outside [1, T_max]");
      total += num_frames[u];
    }
    n->activate();
    const int D = n->nnet.InputDim();
    if (n->nnet.NumSplice() > 1) {
      // a network with frame context pads every utterance at its own ends
      // (pad_input = true): one utterance at a time through kctc_am_nnet_decodable
      long off = 0;
      for (int u = 0; u < N; u++) {
        const int T = num_frames[u];
        n->dec_gather.ensure(sizeof(float) * (size_t)T * D);
        KCTC_HIP_CHECK(hipMemcpy2DAsync(n->dec_gather.p, sizeof(float) * D, feats_dev + (size_t)u * D,
                                        sizeof(float) * (size_t)N * D, sizeof(float) * D, T,
                                        hipMemcpyDeviceToDevice, n->stream));
        const int A = n->nnet.OutputDim();
        if (kctc_am_nnet_decodable(n, n->dec_gather.f(), T, prob_scale, blank_threshold, out_host + off * A,
                                   &rows[u]))
          throw std::runtime_error(kctc_last_error());
        off += rows[u];
      }
      return;
    }
    kctc::SeqLens lens;
    KCTC_REQUIRE(kctc::seq_lens(num_frames, T_max, N, &lens), "kctc_am_nnet_decodable_batch: more than 64 utterances");
    const auto &o = n->evaluator.ForwardSeq(feats_dev, T_max, N, num_frames);
    const int A = o.NumCols();
    const float *pd = device_priors(n, A);
    n->dec_out.ensure(sizeof(float) * (size_t)total * A);
    n->dec_scratch.ensure(kctc::seq_decodable_scratch_bytes(T_max, N));
    n->dec_kept.ensure(sizeof(int) * kctc::kSeqMaxN);
    int *kept_dev = static_cast<int *>(n->dec_kept.p);
    kctc::seq_decodable(n->stream, o.Data(), T_max, N, A, lens, pd, prob_scale, blank_threshold, 1.0e-10f,
                        n->dec_out.f(), n->dec_scratch.p, kept_dev);
    KCTC_HIP_CHECK(hipMemcpyAsync(rows, kept_dev, sizeof(int) * N, hipMemcpyDeviceToHost, n->stream));
    KCTC_HIP_CHECK(hipStreamSynchronize(n->stream));
    collect_profile(n);
    long kept = 0;
    for (int u = 0; u < N; u++) kept += rows[u];
    KCTC_REQUIRE(kept <= total, "kctc_am_nnet_decodable_batch: kept more rows than frames");
    KCTC_HIP_CHECK(hipMemcpy(out_host, n->dec_out.p, sizeof(float) * (size_t)kept * A, hipMemcpyDeviceToHost));
  });
}

int kctc_nnet_sum_posteriors(kctcNnet_t n, const char *rspecifier, int minibatch_size, double *sum, int A,
                             long *frames, long *num_egs) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n && rspecifier && sum, "kctc_nnet_sum_posteriors: null argument");
    KCTC_REQUIRE(minibatch_size >= 1 && minibatch_size <= kctc::kSeqMaxN,
                 "kctc_nnet_sum_posteriors: minibatch_size outside [1, 64]");
    KCTC_REQUIRE(A == n->nnet.OutputDim(), "kctc_nnet_sum_posteriors: A != network output dimension");
    n->activate();
    n->post_sum.ensure(sizeof(double) * A);
    KCTC_HIP_CHECK(hipMemsetAsync(n->post_sum.p, 0, sizeof(double) * A, n->stream));
    long nf = 0;
    const long ne = for_each_batch(rspecifier, minibatch_size, [&](std::vector<kctc::egs::Example> &batch) {
      // every example from its own start offset (eg.left_context - nnet.LeftContext()), pad_input = false
      std::unique_ptr<kctc::egs::Minibatch> mb =
          kctc::egs::pack_minibatch(batch, n->nnet.LeftContext(), n->nnet.RightContext(), true);
      n->check_input_dim(*mb);
      kctc::SeqLens lens;
      if (!kctc::seq_lens(mb->num_frames.data(), mb->T_max, mb->N, &lens))
        throw std::invalid_argument("an example is shorter than the network's context");
      n->stage_minibatch(*mb);
      const auto &o = n->evaluator.ForwardSeq(n->egs_feats.f(), mb->T_max, mb->N, mb->num_frames.data());
      n->post_scratch.ensure(kctc::seq_post_sum_scratch_bytes(mb->T_max, mb->N, A));
      kctc::seq_post_sum(n->stream, o.Data(), mb->T_max, mb->N, A, lens, static_cast<double *>(n->post_sum.p),
                         n->post_scratch.p);
      for (int f : mb->num_frames) nf += f;
    });
    KCTC_HIP_CHECK(hipMemcpyAsync(sum, n->post_sum.p, sizeof(double) * A, hipMemcpyDeviceToHost, n->stream));
    KCTC_HIP_CHECK(hipStreamSynchronize(n->stream));
    collect_profile(n);
    if (frames) *frames = nf;
    if (num_egs) *num_egs = ne;
  });
}

int kctc_am_nnet_adjust_priors(kctcNnet_t n, const double *posterior_sum, int A, float google_prior_const) {
  return kctc_guarded([&] {  // nnet-adjust-priors.cc:126-140
    KCTC_REQUIRE(n, "kctc_am_nnet_adjust_priors: null argument");
    KCTC_REQUIRE(A == n->nnet.OutputDim(), "kctc_am_nnet_adjust_priors: A != number of pdfs");
    std::vector<float> p((size_t)A, 1.0f);
    if (google_prior_const != 0.f) {
      p[0] = google_prior_const;  // un-normalised, as the reference leaves it
    } else {
      KCTC_REQUIRE(posterior_sum, "kctc_am_nnet_adjust_priors: null posterior sum");
      double tot = 0.0;
      for (int a = 0; a < A; a++) tot += posterior_sum[a];
      KCTC_REQUIRE(tot > 0.0, "kctc_am_nnet_adjust_priors: the posterior sum must be positive");
      for (int a = 0; a < A; a++) p[a] = (float)(posterior_sum[a] / tot);
    }
    n->priors = p;
  });
}

int kctc_nnet_compute_prob(kctcNnet_t n, const char *rspecifier, long *num_examples, double *tot_like,
                           double *tot_accuracy, double *tot_weight) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n && rspecifier, "kctc_nnet_compute_prob: null argument");
    n->activate();
    double like = 0, acc = 0, w = 0;
    // ComputeNnetObjf on batches of 10 (ctc-nnet-update.cc:426-431)
    const long ne = for_each_batch(rspecifier, 10, [&](std::vector<kctc::egs::Example> &batch) {
      std::unique_ptr<kctc::egs::Minibatch> mb =
          kctc::egs::pack_minibatch(batch, n->nnet.LeftContext(), n->nnet.RightContext());
      n->stage_minibatch(*mb);
      const auto st = n->evaluator.ComputeForMinibatch(n->egs_feats.f(), mb->T_max, mb->N, mb->num_frames.data(),
                                                       mb->labels.data(), mb->label_lengths.data());
      like += st.tot_objf;
      acc += st.tot_accuracy;
      w += st.tot_weight;  // TotalNnetTrainingWeight: sum of label counts
    });
    if (num_examples) *num_examples = ne;
    if (tot_like) *tot_like = like;
    if (tot_accuracy) *tot_accuracy = acc;
    if (tot_weight) *tot_weight = w;
  });
}

}  // extern "C"
