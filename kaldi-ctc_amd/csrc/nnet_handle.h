// nnet_handle.h -- the object behind the kctcNnet_t handle of
// include/kaldi_ctc_train.h and what the C-ABI sources share: the streams a
// handle owns and the exception mapper.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "common.h"
#include "egs.h"
#include "kaldi_ctc_train.h"
#include "nnet.h"

// The streams of a network or standalone-component handle.  The owner's
// destructor calls quiesce / destroy in the order its other members need.
struct kctcStreams {
  enum { kCompute = 1, kSide = 2, kAll = 3 };
  int device = 0;
  hipStream_t stream = nullptr, side = nullptr, stream2 = nullptr;
  // this handle's device and streams become the calling thread's CuDevice
  void activate() {
    KCTC_HIP_CHECK(hipSetDevice(device));
    auto &d = kctc::nnet2::CuDevice::Instantiate();
    d.device = device;
    d.stream = stream;
    d.side = side;
    d.stream2 = stream2;
  }
  void sync() {
    for (hipStream_t s : {side, stream2, stream})
      if (s) KCTC_HIP_CHECK(hipStreamSynchronize(s));
  }
  // waits for the streams of `part` and takes them out of the thread's CuDevice
  void quiesce(int part) {
    auto &d = kctc::nnet2::CuDevice::Instantiate();
    if ((part & kCompute) && stream) (void)hipStreamSynchronize(stream);
    if ((part & kSide) && side) (void)hipStreamSynchronize(side);
    if ((part & kSide) && stream2) (void)hipStreamSynchronize(stream2);
    if ((part & kCompute) && d.stream == stream) d.stream = nullptr;
    if ((part & kSide) && d.side == side) d.side = nullptr;
    if ((part & kSide) && d.stream2 == stream2) d.stream2 = nullptr;
  }
  void destroy(int part) {
    if ((part & kCompute) && stream) (void)hipStreamDestroy(stream);
    if ((part & kSide) && side) (void)hipStreamDestroy(side);
    if ((part & kSide) && stream2) (void)hipStreamDestroy(stream2);
  }
};

struct kctcNnetImpl : kctcStreams {
  kctc::nnet2::Nnet nnet;
  kctc::nnet2::NnetCtcUpdater trainer{&nnet, true};
  kctc::nnet2::NnetCtcUpdater evaluator{&nnet, false};
  kctc::nnet2::GradExchange *dp = nullptr;
  bool dp_average = false;  // model averaging: no per-step gradient exchange
  kctc::nnet2::DevBuf egs_feats, egs_scratch;  // stage_minibatch
  // decodable (per utterance): device priors, uploaded again only when they
  // change, and the output / scratch buffers, grown and kept
  kctc::nnet2::DevBuf dec_priors, dec_out, dec_scratch, dec_input;
  std::vector<float> dec_priors_host;
  // batched decodable / posterior sum (kaldi_ctc_decode.h): one utterance of a
  // batch gathered for a spliced network, the per-utterance row counts, the
  // fp64 column sums and their slab partials
  kctc::nnet2::DevBuf dec_gather, dec_kept, post_sum, post_scratch;
  // forced alignment (kctc_nnet_align): workspace, frame ids, path scores
  kctc::nnet2::DevBuf ali_ws, ali_ids, ali_scores;
  // prefix beam search (kctc_nnet_decode): workspace, hypotheses, their lengths, scores
  kctc::nnet2::DevBuf beam_ws, beam_hyp, beam_len, beam_scores;
  // graph search (kctc_nnet_decode_graph): posteriors of a network without a final
  // softmax, workspace, words, their counts, frame ilabels, scores, status
  kctc::nnet2::DevBuf wfst_probs, wfst_ws, wfst_words, wfst_len, wfst_ali, wfst_scores, wfst_status;
  // nnet2-ctc model file extras: the CtcTransitionModel exactly as read (opaque
  // bytes, in the mode of the file it came from) and AmNnet's priors
  std::string trans_model;
  bool trans_model_binary = false;
  std::vector<float> priors;
  ~kctcNnetImpl() {
    delete dp;
    quiesce(kAll);
    destroy(kAll);
  }
  // compute stream at the highest priority (the latency-bound recurrences),
  // the weight-gradient side stream at the lowest (nnet_api.cpp)
  void create_streams();
  // an egs minibatch formatted into egs_feats on the compute stream, after
  // the check that its input dimension is the network's (train_api.cpp); a
  // caller with checks of its own between the two makes that one first
  void check_input_dim(const kctc::egs::Minibatch &mb) const;
  void stage_minibatch(kctc::egs::Minibatch &mb);
};

// CUs this process may use when ranks share a device, 0: all (nnet_api.cpp)
int kctc_usable_cus_override();

// kctc_last_error() text of the calling thread (nnet_api.cpp)
void kctc_set_error(const char *msg);

// runs f, mapping exceptions to a non-zero return and kctc_last_error()
template <typename F>
int kctc_guarded(F f) {
  try {
    f();
    return 0;
  } catch (const std::exception &e) {
    kctc_set_error(e.what());
    return 1;
  } catch (...) {
    kctc_set_error("unknown error");
    return 1;
  }
}
