// train_api.cpp -- C ABI of include/kaldi_ctc_train.h, training: the train
// step (synchronous and queued), TrainNnetSimple over an egs reader, data
// parallelism, FormatNnetInput and the synthetic minibatch generator.
#include "kaldi_ctc_train.h"

#include <cmath>
#include <cstring>

#include "grad_exchange.h"
#include "nnet_handle.h"

// the egs minibatch paths' staging (TrainNnetSimple, posterior sums, compute-prob)
void kctcNnetImpl::check_input_dim(const kctc::egs::Minibatch &mb) const {
  if (mb.InputDim() != nnet.InputDim())
    throw std::invalid_argument("egs input dim " + std::to_string(mb.InputDim()) + " != nnet input dim " +
                                std::to_string(nnet.InputDim()));
}
void kctcNnetImpl::stage_minibatch(kctc::egs::Minibatch &mb) {
  check_input_dim(mb);
  egs_feats.ensure(sizeof(float) * (size_t)mb.T_max * mb.N * mb.num_splice * mb.InputDim());
  egs_scratch.ensure(kctc::egs::format_scratch_bytes(mb));
  kctc::egs::format_on_device(mb, egs_feats.f(), egs_scratch.p, egs_scratch.bytes, stream);
}

static void put_stats(const kctc::nnet2::MinibatchStats &st, double *tot_objf, double *tot_accuracy,
                      double *tot_weight) {
  if (tot_objf) *tot_objf = st.tot_objf;
  if (tot_accuracy) *tot_accuracy = st.tot_accuracy;
  if (tot_weight) *tot_weight = st.tot_weight;
}

extern "C" {

int kctc_nnet_last_best_path(kctcNnet_t n, int *ids, long len) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n && ids, "null argument");
    const auto &v = n->trainer.LastBestPath();
    KCTC_REQUIRE(len == (long)v.size(), "kctc_nnet_last_best_path: len != T_max*N of the last minibatch");
    std::copy(v.begin(), v.end(), ids);
  });
}

int kctc_nnet_last_costs(kctcNnet_t n, double *costs, int N) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n && costs, "null argument");
    const auto &v = n->trainer.LastCosts();
    KCTC_REQUIRE(N == (int)v.size(), "kctc_nnet_last_costs: N != minibatch of the last minibatch");
    std::copy(v.begin(), v.end(), costs);
  });
}

int kctc_nnet_last_output(kctcNnet_t n, float *host, long len) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n && host, "null argument");
    n->activate();
    const auto &o = n->trainer.Output();
    KCTC_REQUIRE(o.Data() && len == o.NumRows() * (long)o.NumCols(),
                 "kctc_nnet_last_output: len != T_max*N*A of the last minibatch");
    KCTC_HIP_CHECK(hipStreamSynchronize(n->stream));
    KCTC_HIP_CHECK(hipMemcpy(host, o.Data(), sizeof(float) * len, hipMemcpyDeviceToHost));
  });
}

int kctc_nnet_train_step(kctcNnet_t n, const float *feats_dev, int T_max, int N,
                         const int *num_frames, const int *flat_labels, const int *label_lengths,
                         double *tot_objf, double *tot_accuracy, double *tot_weight) {
  return kctc_guarded([&] {
    n->activate();
    put_stats(n->trainer.ComputeForMinibatch(feats_dev, T_max, N, num_frames, flat_labels, label_lengths), tot_objf,
              tot_accuracy, tot_weight);
  });
}

int kctc_nnet_train_step_async(kctcNnet_t n, const float *feats_dev, int T_max, int N,
                               const int *num_frames, const int *flat_labels, const int *label_lengths,
                               int *have_stats, double *tot_objf, double *tot_accuracy, double *tot_weight) {
  return kctc_guarded([&] {
    n->activate();
    if (have_stats) *have_stats = 0;
    n->trainer.Enqueue(feats_dev, T_max, N, num_frames, flat_labels, label_lengths);
    if (n->trainer.Pending() == 2) {
      put_stats(n->trainer.Finish(), tot_objf, tot_accuracy, tot_weight);
      if (have_stats) *have_stats = 1;
    }
  });
}

int kctc_nnet_train_flush(kctcNnet_t n, int *have_stats, double *tot_objf, double *tot_accuracy,
                          double *tot_weight) {
  return kctc_guarded([&] {
    n->activate();
    if (have_stats) *have_stats = 0;
    if (n->trainer.Pending()) {
      put_stats(n->trainer.Finish(), tot_objf, tot_accuracy, tot_weight);
      if (have_stats) *have_stats = 1;
    }
  });
}

int kctc_nnet_compute_objf(kctcNnet_t n, const float *feats_dev, int T_max, int N,
                           const int *num_frames, const int *flat_labels, const int *label_lengths,
                           double *tot_objf, double *tot_accuracy, double *tot_weight) {
  return kctc_guarded([&] {
    n->activate();
    put_stats(n->evaluator.ComputeForMinibatch(feats_dev, T_max, N, num_frames, flat_labels, label_lengths),
              tot_objf, tot_accuracy, tot_weight);
  });
}

int kctc_nnet_set_length_aware(kctcNnet_t n, int on) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n && (on == 0 || on == 1), "kctc_nnet_set_length_aware: on must be 0 or 1");
    KCTC_REQUIRE(n->trainer.Pending() == 0 && n->evaluator.Pending() == 0,
                 "kctc_nnet_set_length_aware with minibatches in flight");
    if (on)
      for (int c = 0; c < n->nnet.NumComponents(); c++)
        if (auto *r = dynamic_cast<kctc::nnet2::CuDNNRecurrentComponent *>(&n->nnet.GetComponent(c)))
          KCTC_REQUIRE(r->Desc().prec == 0,
                       "kctc_nnet_set_length_aware: bf16 precision is set (it has no length-aware training)");
    n->trainer.SetLengthAware(on != 0);
    n->evaluator.SetLengthAware(on != 0);
  });
}

int kctc_nnet_enable_dp(kctcNnet_t n, const void *uid128, int rank, int world_size) {
  return kctc_guarded([&] {
    n->activate();
    KCTC_REQUIRE(world_size >= 0 && (world_size == 0 || (rank >= 0 && rank < world_size && uid128)),
                 "kctc_nnet_enable_dp: bad rank / world size");
    KCTC_REQUIRE(n->trainer.Pending() == 0, "kctc_nnet_enable_dp with minibatches in flight");
    delete n->dp;
    n->dp = nullptr;
    n->trainer.SetExchange(nullptr);
    if (world_size >= 1) {  // one rank included: the same communicator and all-reduce path
      n->dp = kctc_new_rccl_exchange(uid128, rank, world_size, n->stream);
      n->trainer.SetExchange(n->dp_average ? nullptr : n->dp);
    }
  });
}

int kctc_nnet_enable_dp_host(kctcNnet_t n, kctc_host_allreduce_fn fn, void *user, int world_size) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n && fn && world_size >= 1, "kctc_nnet_enable_dp_host: bad argument");
    KCTC_REQUIRE(n->trainer.Pending() == 0, "kctc_nnet_enable_dp_host with minibatches in flight");
    n->activate();
    delete n->dp;
    n->dp = nullptr;
    n->trainer.SetExchange(nullptr);
    n->dp = kctc_new_host_exchange(fn, user, world_size, n->stream);
    n->trainer.SetExchange(n->dp_average ? nullptr : n->dp);
  });
}

int kctc_nnet_enable_cu_probe(kctcNnet_t n, int blocks, double usec) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n && blocks >= 0 && usec >= 0, "kctc_nnet_enable_cu_probe: bad argument");
    KCTC_REQUIRE(n->trainer.Pending() == 0, "kctc_nnet_enable_cu_probe with minibatches in flight");
    n->activate();
    delete n->dp;
    n->dp = nullptr;
    n->trainer.SetExchange(nullptr);
    if (blocks > 0) {
      n->dp = kctc_new_cu_probe_exchange(blocks, usec, n->stream);
      n->trainer.SetExchange(n->dp);
    }
  });
}

int kctc_nnet_inject_step_error(kctcNnet_t n, unsigned word) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n, "null nnet");
    n->trainer.InjectStepError(word);
  });
}

int kctc_nnet_set_dp_mode(kctcNnet_t n, int mode) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n && (mode == 0 || mode == 1), "kctc_nnet_set_dp_mode: mode must be 0 or 1");
    KCTC_REQUIRE(n->trainer.Pending() == 0, "kctc_nnet_set_dp_mode with minibatches in flight");
    n->dp_average = mode == 1;
    n->trainer.SetExchange(n->dp && !n->dp_average ? n->dp : nullptr);
  });
}

// nnet-am-average over the data-parallel ranks (src/nnet2bin/nnet-am-average.cc:
// 185-241 with the default weights 1/num-models), on the component API the tool
// uses: every rank's updatable component is Scale(1/world)d (the tool's scale
// of model 1 by its weight), then the collective sum adds the other ranks'
// scaled copies (the tool's Add(weight, model i)), on the compute stream.
int kctc_nnet_average_params(kctcNnet_t n) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n && n->dp, "kctc_nnet_average_params: data parallelism not enabled");
    KCTC_REQUIRE(n->trainer.Pending() == 0, "kctc_nnet_average_params with minibatches in flight");
    n->activate();
    const int world = n->dp->WorldSize();
    for (int c = 0; c < n->nnet.NumComponents(); c++) {
      // the tool's NonlinearComponent share: RectifiedLinear's statistics
      // (a sum over one rank is the identity, and exact)
      if (auto *rl = dynamic_cast<kctc::nnet2::RectifiedLinearComponent *>(&n->nnet.GetComponent(c))) {
        if (world > 1) {
          rl->Scale(1.f / (float)world);
          rl->AllReduceStats(*n->dp, n->stream);
        }
        continue;
      }
      auto *u = dynamic_cast<kctc::nnet2::UpdatableComponent *>(&n->nnet.GetComponent(c));
      if (!u) continue;
      if (world > 1) u->Scale(1.f / (float)world);
      n->dp->AllReduceSum(u->ParamData(), u->NumParameters(), n->stream);
    }
    KCTC_HIP_CHECK(hipStreamSynchronize(n->stream));
  });
}

int kctc_nnet_train_simple(kctcNnet_t n, struct kctcEgsReader_ *r, long max_minibatches, long *num_egs,
                           double *tot_weight, double *tot_objf, double *tot_accuracy) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n && r, "kctc_nnet_train_simple: null argument");
    n->activate();
    long egs = 0, mbs = 0;
    double w = 0, objf = 0, acc = 0;
    while (max_minibatches <= 0 || mbs < max_minibatches) {
      std::unique_ptr<kctc::egs::Minibatch> mb = r->r.Next();  // GetNextMinibatch
      if (!mb) break;
      n->check_input_dim(*mb);
      if (mb->num_splice != n->nnet.NumSplice())
        throw std::invalid_argument("the egs reader was opened with a context other than the network's "
                                    "(kctc_nnet_context)");
      n->stage_minibatch(*mb);
      const auto st = n->trainer.ComputeForMinibatch(n->egs_feats.f(), mb->T_max, mb->N, mb->num_frames.data(),
                                                     mb->labels.data(), mb->label_lengths.data());
      objf += st.tot_objf;
      acc += st.tot_accuracy;
      w += st.tot_weight;
      egs += mb->N;
      mbs++;
    }
    if (num_egs) *num_egs = egs;
    if (tot_weight) *tot_weight = w;
    if (tot_objf) *tot_objf = objf;
    if (tot_accuracy) *tot_accuracy = acc;
  });
}

int kctc_levenshtein(const int *ref, int nref, const int *hyp, int nhyp) {
  if ((nref > 0 && !ref) || (nhyp > 0 && !hyp)) return -1;
  return kctc::nnet2::levenshtein(ref, nref, hyp, nhyp);
}

int kctc_format_input(const float *feats, const int *num_frames, int N, int dim, int T_max,
                      float *out) {
  return kctc_guarded([&] {
    // FormatNnetInput (ctc-nnet-update.cc:351-424): row t*N+n, zero padded
    memset(out, 0, sizeof(float) * (size_t)T_max * N * dim);
    long off = 0;
    for (int n = 0; n < N; n++) {
      if (num_frames[n] > T_max) throw std::invalid_argument("num_frames > T_max");
      for (int t = 0; t < num_frames[n]; t++)
        memcpy(out + ((size_t)t * N + n) * dim, feats + (off + t) * (size_t)dim, sizeof(float) * dim);
      off += num_frames[n];
    }
  });
}

long kctc_synth_minibatch(unsigned long long seed, int T_max, int N, int dim, int A,
                          double label_ratio, float *feats, int *num_frames, int *flat_labels,
                          int *label_lengths) {
  kctc::nnet2::Rng rng(seed);
  long nl = 0;
  for (int n = 0; n < N; n++) {
    int T = n == 0 ? T_max : T_max - (int)std::floor(rng.uniform() * 0.1 * T_max);
    if (T < 1) T = 1;
    num_frames[n] = T;
    long L = (long)std::floor(T * label_ratio);
    L = std::min<long>(L, 639);
    L = std::min<long>(L, (T - 1) / 2);
    L = std::max<long>(L, 0);
    label_lengths[n] = (int)L;
    int prev = -1;
    for (long i = 0; i < L; i++) {
      int v;
      do {
        v = 1 + (int)(rng.next() % (unsigned long long)(A - 1));
      } while (v == prev && A > 2);
      flat_labels[nl++] = v;
      prev = v;
    }
  }
  if (feats) {
    for (int t = 0; t < T_max; t++)
      for (int n = 0; n < N; n++) {
        float *row = feats + ((size_t)t * N + n) * dim;
        if (t < num_frames[n])
          for (int j = 0; j < dim; j++) row[j] = (float)rng.gauss();
        else
          memset(row, 0, sizeof(float) * dim);
      }
  }
  return nl;
}

}  // extern "C"
