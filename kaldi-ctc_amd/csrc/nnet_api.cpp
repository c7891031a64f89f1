// nnet_api.cpp -- C ABI of include/kaldi_ctc_train.h, the handle itself: its
// lifetime and streams, the CU partition, the error text, parameter and
// settings accessors, profiling and model files.
#include "kaldi_ctc_train.h"

#include <algorithm>
#include <cstring>
#include <sstream>

#include "elementwise.h"
#include "kaldi_io.h"
#include "nnet_handle.h"

using kctc::nnet2::CuDevice;

static thread_local std::string g_err;
void kctc_set_error(const char *msg) { g_err = msg ? msg : ""; }

// CUs of the device this process may use: all of them, or its share when
// ranks share a device (kctc_set_cu_partition)
static int g_part = 0, g_nparts = 1;
int kctc_usable_cus_override() {
  if (g_nparts <= 1) return 0;
  int dev = 0, cus = 0;
  KCTC_HIP_CHECK(hipGetDevice(&dev));
  KCTC_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  return cus / g_nparts;
}

// the CU mask of share `part` of `nparts`: a contiguous range of mask bits
// (bit b: one CU of XCD b mod 8, scripts/cumask_probe.hip)
static std::vector<uint32_t> partition_mask(int part, int nparts, int cus) {
  const int per = cus / nparts, first = part * per;
  std::vector<uint32_t> mask((cus + 31) / 32, 0u);
  for (int c = first; c < first + per; c++) mask[c / 32] |= 1u << (c % 32);
  return mask;
}

// compute stream at the highest priority (the latency-bound recurrences),
// the weight-gradient side stream at the lowest, and a default-priority
// queue for the streamed GEMMs
void kctcNnetImpl::create_streams() {
  if (g_nparts > 1) {  // ranks sharing the device: this rank's streams on its CU share only
    int cus = 0;
    KCTC_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    const int per = cus / g_nparts;
    const std::vector<uint32_t> mask = partition_mask(g_part, g_nparts, cus);
    KCTC_HIP_CHECK(hipExtStreamCreateWithCUMask(&stream, (uint32_t)mask.size(), mask.data()));
    KCTC_HIP_CHECK(hipExtStreamCreateWithCUMask(&side, (uint32_t)mask.size(), mask.data()));
    KCTC_HIP_CHECK(hipExtStreamCreateWithCUMask(&stream2, (uint32_t)mask.size(), mask.data()));
    kctc::rnn_set_cu_budget(per, kctc::rnn_comm_cus());
    return;
  }
  int lo = 0, hi = 0;
  KCTC_HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
  KCTC_HIP_CHECK(hipStreamCreateWithPriority(&stream, hipStreamNonBlocking, hi));
  KCTC_HIP_CHECK(hipStreamCreateWithPriority(&side, hipStreamNonBlocking, lo));
  // streamed GEMMs (default priority: a queue of its own, neither the recurrences' nor the side stream's)
  KCTC_HIP_CHECK(hipStreamCreateWithFlags(&stream2, hipStreamNonBlocking));
}

// a handle with its streams on `device`, filled in by `fill`; nothing is left
// behind when that throws
template <typename F>
static int new_on_device(kctcNnet_t *out, int device, F fill) {
  return kctc_guarded([&] {
    std::unique_ptr<kctcNnetImpl> n(new kctcNnetImpl);
    n->device = device;
    KCTC_HIP_CHECK(hipSetDevice(device));
    n->create_streams();
    n->activate();
    fill(n.get());
    *out = n.release();
  });
}

static kctc::nnet2::Component &comp(kctcNnet_t n, int c) {
  if (c < 0 || c >= n->nnet.NumComponents()) throw std::out_of_range("component index");
  return n->nnet.GetComponent(c);
}
static kctc::nnet2::UpdatableComponent &ucomp(kctcNnet_t n, int c) {
  auto &x = comp(n, c);
  if (!x.IsUpdatable()) throw std::invalid_argument("component is not updatable");
  return static_cast<kctc::nnet2::UpdatableComponent &>(x);
}

extern "C" {

const char *kctc_last_error(void) { return g_err.c_str(); }

int kctc_nnet_create(kctcNnet_t *out, const char *config, unsigned long long seed, int device) {
  return new_on_device(out, device, [&](kctcNnetImpl *n) {
    kctc::nnet2::Rng rng(seed);
    n->nnet.Init(config ? config : "", rng);
    n->nnet.SetDropoutSeed(seed);  // a stream of its own: not the parameters' rng, not rand()
  });
}

int kctc_nnet_destroy(kctcNnet_t n) {
  return kctc_guarded([&] {
    if (n) {
      n->activate();
      KCTC_HIP_CHECK(hipStreamSynchronize(n->stream));
    }
    delete n;
  });
}

int kctc_nnet_num_components(kctcNnet_t n) { return n ? n->nnet.NumComponents() : -1; }

int kctc_nnet_context(kctcNnet_t n, int *left, int *right) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n && left && right, "kctc_nnet_context: null argument");
    *left = n->nnet.LeftContext();
    *right = n->nnet.RightContext();
  });
}

int kctc_nnet_component_info(kctcNnet_t n, int c, char *buf, size_t len) {
  return kctc_guarded([&] {
    n->activate();
    std::string s = comp(n, c).Info();
    if (len) {
      strncpy(buf, s.c_str(), len - 1);
      buf[len - 1] = 0;
    }
  });
}

long kctc_nnet_num_params(kctcNnet_t n, int c) {
  if (!n || c < 0 || c >= n->nnet.NumComponents() || !n->nnet.GetComponent(c).IsUpdatable()) return 0;
  return static_cast<kctc::nnet2::UpdatableComponent &>(n->nnet.GetComponent(c)).NumParameters();
}

int kctc_nnet_get_params(kctcNnet_t n, int c, float *host, long len) {
  return kctc_guarded([&] {
    n->activate();
    auto &u = ucomp(n, c);
    if (len != u.NumParameters()) throw std::invalid_argument("size mismatch");
    u.Vectorize(host);
  });
}

int kctc_nnet_set_params(kctcNnet_t n, int c, const float *host, long len) {
  return kctc_guarded([&] {
    n->activate();
    auto &u = ucomp(n, c);
    if (len != u.NumParameters()) throw std::invalid_argument("size mismatch");
    u.UnVectorize(host);
  });
}

int kctc_nnet_get_grad(kctcNnet_t n, int c, float *host, long len) {
  return kctc_guarded([&] {
    n->activate();
    auto &u = ucomp(n, c);
    if (len != u.NumParameters()) throw std::invalid_argument("size mismatch");
    KCTC_HIP_CHECK(hipStreamSynchronize(n->stream));
    KCTC_HIP_CHECK(hipStreamSynchronize(u.GradStream()));
    KCTC_HIP_CHECK(hipMemcpy(host, u.GradData(), sizeof(float) * len, hipMemcpyDeviceToHost));
  });
}

int kctc_nnet_set_learning_rate(kctcNnet_t n, float lr) {
  return kctc_guarded([&] { n->nnet.SetLearningRate(lr); });
}

int kctc_nnet_clip_stats(kctcNnet_t n, int c, double *num_clipped, double *count) {
  return kctc_guarded([&] {
    n->activate();
    auto *cg = dynamic_cast<kctc::nnet2::ClipGradientComponent *>(&comp(n, c));
    if (!cg) throw std::invalid_argument("not a ClipGradientComponent");
    cg->SyncStats();
    *num_clipped = cg->NumClipped();
    *count = cg->Count();
  });
}

int kctc_nnet_srand(kctcNnet_t n, unsigned seed) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n, "null nnet");
    n->trainer.Srand(seed);
  });
}

int kctc_nnet_rand_calls(kctcNnet_t n, long *calls) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n && calls, "null argument");
    *calls = n->trainer.RandCalls();
  });
}

struct ihipStream_t *kctc_nnet_stream(kctcNnet_t n) { return n ? n->stream : nullptr; }

int kctc_nnet_set_profiling(kctcNnet_t n, int on) {
  return kctc_guarded([&] {
    n->activate();
    auto &d = CuDevice::Instantiate();
    d.profiling = on != 0;
    d.prof.clear();
  });
}

int kctc_nnet_profile(kctcNnet_t n, const char *family, double *ms_total, int *launches) {
  return kctc_guarded([&] {
    auto &d = CuDevice::Instantiate();
    auto it = d.prof.find(family ? family : "");
    *ms_total = it == d.prof.end() ? 0.0 : it->second.first;
    *launches = it == d.prof.end() ? 0 : it->second.second;
  });
}

int kctc_nnet_write(kctcNnet_t n, const char *path) { return kctc_nnet_write_kaldi(n, path, 0); }

int kctc_nnet_write_kaldi(kctcNnet_t n, const char *path, int binary) {
  return kctc_guarded([&] {
    n->activate();
    kctc::kio::WriteFile(path, binary != 0, [&](std::ostream &os) { n->nnet.Write(os, binary != 0); });
  });
}

// whole file in memory (models are ~0.1 GB); `am`: the nnet2-ctc model form
// (CtcTransitionModel + Nnet + priors, nnet2-ctc-train-simple.cc:58-64)
static void read_model(kctcNnetImpl *n, const char *path, bool am) {
  std::istringstream is(kctc::kio::ReadFile(path));
  const bool binary = kctc::kio::InitInput(is);
  if (am && kctc::kio::PeekToken(is, binary) == "<TransitionModel>") {
    // kept opaque: everything up to and including the "</TransitionModel> " token
    const std::string &buf = is.str();
    const std::string end_tok = "</TransitionModel> ";
    const auto start = (size_t)is.tellg();
    const auto e = buf.find(end_tok, start);
    if (e == std::string::npos) throw std::runtime_error("unterminated <TransitionModel>");
    // text mode: TransitionModel::Write ends the token with a newline
    // (src/hmm/transition-model.cc:316-317); keep it, so write-back is byte-identical
    size_t stop = e + end_tok.size();
    if (!binary && stop < buf.size() && buf[stop] == '\n') stop++;
    n->trans_model = buf.substr(start, stop - start);
    n->trans_model_binary = binary;
    is.seekg((std::streamoff)stop);
  }
  n->nnet.Read(is, binary);
  if (am) {
    n->priors = kctc::kio::ReadFloatVector(is, binary);
    if (!n->priors.empty() && (int)n->priors.size() != n->nnet.OutputDim())
      throw std::runtime_error("AmNnet priors dimension != network output dimension");
  }
}

int kctc_nnet_read(kctcNnet_t *out, const char *path, int device) {
  return new_on_device(out, device, [&](kctcNnetImpl *n) { read_model(n, path, false); });
}

int kctc_am_nnet_read(kctcNnet_t *out, const char *path, int device) {
  return new_on_device(out, device, [&](kctcNnetImpl *n) { read_model(n, path, true); });
}

int kctc_am_nnet_write(kctcNnet_t n, const char *path, int binary) {
  return kctc_guarded([&] {
    n->activate();
    if (!n->trans_model.empty() && n->trans_model_binary != (binary != 0))
      throw std::runtime_error("the transition model was read in the other mode; write the model in that mode");
    kctc::kio::WriteFile(path, binary != 0, [&](std::ostream &os) {
      os.write(n->trans_model.data(), (std::streamsize)n->trans_model.size());
      n->nnet.Write(os, binary != 0);
      kctc::kio::WriteFloatVector(os, binary != 0, n->priors.data(), (long)n->priors.size());
    });
  });
}

int kctc_am_nnet_num_priors(kctcNnet_t n) { return n ? (int)n->priors.size() : -1; }

int kctc_am_nnet_get_priors(kctcNnet_t n, float *priors, int dim) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(dim == (int)n->priors.size() && (dim == 0 || priors), "kctc_am_nnet_get_priors: bad size");
    std::copy(n->priors.begin(), n->priors.end(), priors);
  });
}

int kctc_am_nnet_set_priors(kctcNnet_t n, const float *priors, int dim) {
  return kctc_guarded([&] {  // AmNnet::SetPriors (am-nnet.cc:44-55)
    const int pdfs = n->nnet.OutputDim();
    KCTC_REQUIRE(dim >= 0 && dim <= pdfs, "Dimension of priors cannot exceed number of pdfs.");
    KCTC_REQUIRE(dim == 0 || priors, "kctc_am_nnet_set_priors: null priors");
    n->priors.assign(priors, priors + dim);
    if (dim > 0 && dim < pdfs) n->priors.resize(pdfs, 0.f);
  });
}

int kctc_set_cu_partition(int part, int nparts) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(nparts >= 1 && nparts <= 8 && part >= 0 && part < nparts, "kctc_set_cu_partition: bad partition");
    g_part = part;
    g_nparts = nparts;
    kctc::rnn_set_cu_budget(kctc_usable_cus_override(), kctc::rnn_comm_cus());
  });
}

int kctc_cu_partition_probe(int part, int nparts, unsigned *ids, int max_ids, int *n_ids) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(nparts >= 1 && nparts <= 8 && part >= 0 && part < nparts && ids && n_ids && max_ids > 0,
                 "kctc_cu_partition_probe: bad arguments");
    int dev = 0, cus = 0;
    KCTC_HIP_CHECK(hipGetDevice(&dev));
    KCTC_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const std::vector<uint32_t> mask = partition_mask(part, nparts, cus);
    hipStream_t s = nullptr;
    KCTC_HIP_CHECK(hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data()));
    const int blocks = 8 * cus;
    unsigned *d = nullptr;
    KCTC_HIP_CHECK(hipMalloc(&d, sizeof(unsigned) * blocks));
    kctc::cu_where(s, d, blocks, 50.0);  // long enough that the blocks spread over every CU of the share
    std::vector<unsigned> h(blocks);
    KCTC_HIP_CHECK(hipMemcpyAsync(h.data(), d, sizeof(unsigned) * blocks, hipMemcpyDeviceToHost, s));
    KCTC_HIP_CHECK(hipStreamSynchronize(s));
    (void)hipFree(d);
    (void)hipStreamDestroy(s);
    std::sort(h.begin(), h.end());
    h.erase(std::unique(h.begin(), h.end()), h.end());
    *n_ids = (int)std::min<size_t>(h.size(), (size_t)max_ids);
    std::copy(h.begin(), h.begin() + *n_ids, ids);
  });
}

int kctc_nnet_set_precision(kctcNnet_t n, int precision) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n && (precision == 0 || precision == 1), "kctc_nnet_set_precision: precision must be 0 or 1");
    KCTC_REQUIRE(n->trainer.Pending() == 0, "kctc_nnet_set_precision with minibatches in flight");
    KCTC_REQUIRE(precision == 0 || !n->trainer.LengthAware(),
                 "kctc_nnet_set_precision: bf16 has no length-aware training (kctc_nnet_set_length_aware is on)");
    for (int c = 0; c < n->nnet.NumComponents(); c++)
      if (auto *r = dynamic_cast<kctc::nnet2::CuDNNRecurrentComponent *>(&n->nnet.GetComponent(c)))
        r->SetPrecision(precision);
  });
}

int kctc_nnet_set_momentum(kctcNnet_t n, float momentum) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n, "null nnet");
    n->activate();
    n->nnet.SetMomentum(momentum);
  });
}

int kctc_nnet_set_dropout_seed(kctcNnet_t n, unsigned long long seed) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n, "null nnet");
    KCTC_REQUIRE(n->trainer.Pending() == 0, "kctc_nnet_set_dropout_seed with minibatches in flight");
    n->nnet.SetDropoutSeed(seed);
  });
}

int kctc_nnet_set_dropout_scale(kctcNnet_t n, float scale) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n, "null nnet");
    KCTC_REQUIRE(n->trainer.Pending() == 0, "kctc_nnet_set_dropout_scale with minibatches in flight");
    n->nnet.SetDropoutScale(scale);
  });
}

int kctc_nnet_remove_dropout(kctcNnet_t n, int *removed) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n, "null nnet");
    KCTC_REQUIRE(n->trainer.Pending() == 0, "kctc_nnet_remove_dropout with minibatches in flight");
    n->activate();
    // the per-component buffers that go away may still be read by queued work
    n->sync();
    const int r = n->nnet.RemoveDropout();
    // momentum shadows and update deltas live in the components that stay, and
    // the gradient exchange registers its buckets anew every step: what is
    // indexed by component is the two updaters' forward data and chunk info
    n->trainer.ComponentsChanged();
    n->evaluator.ComponentsChanged();
    if (removed) *removed = r;
  });
}

int kctc_nnet_insert(kctcNnet_t n, int insert_at, const char *config, unsigned long long seed) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(n && config, "kctc_nnet_insert: null argument");
    KCTC_REQUIRE(n->trainer.Pending() == 0 && n->evaluator.Pending() == 0,
                 "kctc_nnet_insert with minibatches in flight");
    n->activate();
    KCTC_HIP_CHECK(hipStreamSynchronize(n->stream));
    if (n->side) KCTC_HIP_CHECK(hipStreamSynchronize(n->side));
    kctc::nnet2::Rng rng(seed);
    n->nnet.Insert(insert_at, config, rng);
    // what is indexed by component: the two updaters' forward data and chunk info
    n->trainer.ComponentsChanged();
    n->evaluator.ComponentsChanged();
    KCTC_HIP_CHECK(hipStreamSynchronize(n->stream));
  });
}

}  // extern "C"
