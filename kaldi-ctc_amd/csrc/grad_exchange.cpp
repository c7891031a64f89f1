// grad_exchange.cpp -- the data-parallel gradient exchanges behind nnet.h's
// GradExchange: RCCL, a host transport, and the CU-budget probe.
#include "grad_exchange.h"

#include <rccl/rccl.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "elementwise.h"
#include "nnet_handle.h"

// Gradient all-reduce over RCCL on a dedicated stream: each component's
// gradient bucket is reduced as soon as its Backprop has produced it, while
// the compute stream goes on with the layers below (overlap); the SGD updates
// wait for the last bucket.  Sum semantics: the summed gradient of the G
// per-rank minibatches equals the gradient of their concatenation, then the
// reference's per-component clip (+-clip-gradient) and SGD run identically
// on every rank, so replicas stay bit-identical.
//
// CU budget: the all-reduces run during the backward pass,
// beside the persistent recurrence and the streamed dx GEMM, whose blocks must
// all be resident.  RCCL's kernels are capped at kctc_comm_ctas() blocks
// (ncclConfig_t.maxCTAs) and the streamed GEMMs leave that many CUs free
// (rnn_set_cu_budget), so even if every RCCL block kept a CU to itself the
// recurrence's workgroups still find theirs.
static int kctc_comm_ctas() {
  const char *e = getenv("KCTC_COMM_CTAS");
  const int v = e && *e ? atoi(e) : 16;
  return std::max(1, std::min(v, 64));
}

namespace {

// Residency-gated exchange: a bucket's reduction is queued on
// the comm stream only behind the NEXT backward recurrence's launch, after a
// gate kernel's wait until every workgroup of that recurrence is resident
// (rnn_comm_gate, its blocks off the recurrence's XCDs; after its end instead
// when it uses scratch, rnn.h rnn_last_bwd_scratch_free), and the launch of the recurrence after that waits
// for it.  So no exchange kernel holds a CU while a recurrence's workgroups
// are being placed -- the condition under which an XCD-pinned recurrence
// (which needs all CUs of its XCDs) could wait on an all-reduce that waits on
// another GPU -- and the backward recurrences stay XCD-pinned with the
// exchange configured (rnn_set_comm_gated).  The last bucket (bottom
// component) goes out at Finish, with no recurrence after it.  KCTC_COMM_GATE=0
// reduces every bucket at once and leaves the backward unpinned (round 3).
class GatedExchange : public kctc::nnet2::GradExchange {
 public:
  GatedExchange(hipStream_t compute, int comm_cus) : compute_(compute) {
    const char *e = getenv("KCTC_COMM_GATE");
    gated_ = !(e && *e == '0');
    // the gate waits on the device's registration word, which every network's
    // backward recurrences add to: two gated exchanges on one device would
    // wait on each other's recurrences
    if (gated_ && kctc::rnn_comm_gated())
      throw std::runtime_error("a gated gradient exchange is already active on this device (one data-parallel "
                               "network per device and process; KCTC_COMM_GATE=0 lifts the limit)");
    kctc::rnn_set_cu_budget(kctc_usable_cus_override(), comm_cus);
    if (gated_) kctc::rnn_set_comm_gated(true);
    KCTC_HIP_CHECK(hipStreamCreateWithFlags(&comm_stream_, hipStreamNonBlocking));
    KCTC_HIP_CHECK(hipEventCreateWithFlags(&done_, hipEventDisableTiming));
    KCTC_HIP_CHECK(hipEventCreateWithFlags(&after_, hipEventDisableTiming));
  }
  ~GatedExchange() override {
    kctc::rnn_set_cu_budget(kctc_usable_cus_override(), 0);
    if (gated_) kctc::rnn_set_comm_gated(false);
    (void)hipStreamSynchronize(comm_stream_);
    (void)hipStreamDestroy(comm_stream_);
    (void)hipEventDestroy(done_);
    (void)hipEventDestroy(after_);
    for (auto ev : pool_) (void)hipEventDestroy(ev);
  }
  void GradReady(int, float *grad, long n, hipStream_t producer) override {
    if (next_ev_ == pool_.size()) {
      hipEvent_t ev;
      KCTC_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      pool_.push_back(ev);
    }
    hipEvent_t ev = pool_[next_ev_++];
    KCTC_HIP_CHECK(hipEventRecord(ev, producer));
    pending_.push_back({grad, n, ev});
    if (!gated_) Launch();
  }
  void BeforeRecurrence(hipStream_t compute) override {
    // the reductions queued behind the previous recurrence ran while it was
    // resident; this launch waits for them (they normally end long before)
    if (gated_ && launched_) KCTC_HIP_CHECK(hipStreamWaitEvent(compute, done_, 0));
    launched_ = false;
  }
  void AfterRecurrence() override {
    if (!gated_ || pending_.empty()) return;
    if (kctc::rnn_last_bwd_scratch_free()) {
      kctc::rnn_comm_gate(comm_stream_, kctc::rnn_bwd_registrations());
    } else {  // nothing beside a recurrence that uses scratch: after its end
      KCTC_HIP_CHECK(hipEventRecord(after_, compute_));
      KCTC_HIP_CHECK(hipStreamWaitEvent(comm_stream_, after_, 0));
    }
    Launch();
  }
  void Finish() override {
    Launch();
    KCTC_HIP_CHECK(hipEventRecord(done_, comm_stream_));
    KCTC_HIP_CHECK(hipStreamWaitEvent(compute_, done_, 0));
    launched_ = false;
    next_ev_ = 0;
  }
  void AllReduceSum(float *buf, long n, hipStream_t s) override {
    KCTC_HIP_CHECK(hipEventRecord(done_, s));
    KCTC_HIP_CHECK(hipStreamWaitEvent(comm_stream_, done_, 0));
    Reduce(buf, n);
    KCTC_HIP_CHECK(hipEventRecord(done_, comm_stream_));
    KCTC_HIP_CHECK(hipStreamWaitEvent(s, done_, 0));
  }

 protected:
  virtual void Reduce(float *buf, long n) = 0;  // in place on comm_stream_
  hipStream_t compute_, comm_stream_ = nullptr;

 private:
  void Launch() {
    if (pending_.empty()) return;
    for (const auto &b : pending_) {
      KCTC_HIP_CHECK(hipStreamWaitEvent(comm_stream_, b.ready, 0));
      Reduce(b.grad, b.n);
    }
    pending_.clear();
    KCTC_HIP_CHECK(hipEventRecord(done_, comm_stream_));
    launched_ = true;
  }
  struct Bucket {
    float *grad;
    long n;
    hipEvent_t ready;
  };
  bool gated_ = true, launched_ = false;
  hipEvent_t done_ = nullptr;
  hipEvent_t after_ = nullptr;  // the end of a recurrence that uses scratch
  std::vector<hipEvent_t> pool_;
  size_t next_ev_ = 0;
  std::vector<Bucket> pending_;
};

class RcclExchange : public GatedExchange {
 public:
  RcclExchange(const void *uid, int rank, int world, hipStream_t compute)
      : GatedExchange(compute, kctc_comm_ctas()), world_(world) {
    ncclUniqueId id;
    memcpy(&id, uid, sizeof(id));
    ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
    cfg.blocking = 1;
    cfg.maxCTAs = kctc_comm_ctas();
    cfg.minCTAs = std::min(cfg.maxCTAs, 4);
    if (ncclCommInitRankConfig(&comm_, world, id, rank, &cfg) != ncclSuccess)
      throw std::runtime_error("ncclCommInitRankConfig failed");
  }
  ~RcclExchange() override {
    (void)hipStreamSynchronize(comm_stream_);
    ncclCommDestroy(comm_);
  }
  int WorldSize() const override { return world_; }

 protected:
  void Reduce(float *buf, long n) override {
    if (ncclAllReduce(buf, buf, (size_t)n, ncclFloat, ncclSum, comm_, comm_stream_) != ncclSuccess)
      throw std::runtime_error("ncclAllReduce failed");
  }

 private:
  int world_;
  ncclComm_t comm_ = nullptr;
};

// The same exchange over a host transport (kctc_nnet_enable_dp_host): the
// buckets are registered in backprop order as with RCCL; Finish() sums each
// one through the caller's all-reduce (device -> pinned host -> all-reduce ->
// device) before the updates.  Host-synchronous: a transport for ranks that
// share a GPU or have no RCCL peer, not the fast path.
class HostExchange : public kctc::nnet2::GradExchange {
 public:
  HostExchange(kctc_host_allreduce_fn fn, void *user, int world, hipStream_t compute)
      : fn_(fn), user_(user), world_(world), compute_(compute) {
    KCTC_HIP_CHECK(hipEventCreateWithFlags(&ev_, hipEventDisableTiming));
  }
  ~HostExchange() override {
    if (host_) (void)hipHostFree(host_);
    (void)hipEventDestroy(ev_);
  }
  void GradReady(int, float *grad, long n, hipStream_t producer) override {
    buckets_.push_back({grad, n, producer});
  }
  void Finish() override {
    for (const auto &b : buckets_) {
      if ((size_t)b.n > cap_) {
        if (host_) KCTC_HIP_CHECK(hipHostFree(host_));
        KCTC_HIP_CHECK(hipHostMalloc((void **)&host_, sizeof(float) * b.n, hipHostMallocDefault));
        cap_ = (size_t)b.n;
      }
      KCTC_HIP_CHECK(hipEventRecord(ev_, b.producer));
      KCTC_HIP_CHECK(hipStreamWaitEvent(compute_, ev_, 0));
      KCTC_HIP_CHECK(hipMemcpyAsync(host_, b.grad, sizeof(float) * b.n, hipMemcpyDeviceToHost, compute_));
      KCTC_HIP_CHECK(hipStreamSynchronize(compute_));
      fn_(host_, b.n, user_);
      KCTC_HIP_CHECK(hipMemcpyAsync(b.grad, host_, sizeof(float) * b.n, hipMemcpyHostToDevice, compute_));
      KCTC_HIP_CHECK(hipStreamSynchronize(compute_));
    }
    buckets_.clear();
  }
  int WorldSize() const override { return world_; }
  void AllReduceSum(float *buf, long n, hipStream_t s) override {
    buckets_.push_back({buf, n, s});
    Finish();
  }

 private:
  struct Bucket {
    float *grad;
    long n;
    hipStream_t producer;
  };
  kctc_host_allreduce_fn fn_;
  void *user_;
  int world_;
  hipStream_t compute_;
  hipEvent_t ev_ = nullptr;
  float *host_ = nullptr;
  size_t cap_ = 0;
  std::vector<Bucket> buckets_;
};

// CU-budget probe (kctc_nnet_enable_cu_probe): a one-rank exchange whose
// "all-reduce" of every gradient bucket is a kernel holding `blocks` whole CUs
// for `usec` on the comm stream -- the worst case of an exchange kernel that
// keeps its CUs to itself while the next component's backward recurrence and
// streamed dx GEMM run.  Gated like RcclExchange (the backward stays pinned);
// the gradients are not touched (a sum over one rank).
class CuProbeExchange : public GatedExchange {
 public:
  CuProbeExchange(int blocks, double usec, hipStream_t compute)
      : GatedExchange(compute, blocks), blocks_(blocks), usec_(usec) {}
  int WorldSize() const override { return 1; }
  void AllReduceSum(float *, long, hipStream_t) override {}
  long launches_ = 0;

 protected:
  void Reduce(float *, long) override {
    kctc::cu_hold(comm_stream_, blocks_, usec_);
    launches_++;
  }

 private:
  int blocks_;
  double usec_;
};

}  // namespace

using kctc::nnet2::GradExchange;
GradExchange *kctc_new_rccl_exchange(const void *uid128, int rank, int world, hipStream_t compute) {
  return new RcclExchange(uid128, rank, world, compute);
}
GradExchange *kctc_new_host_exchange(kctc_host_allreduce_fn fn, void *user, int world, hipStream_t compute) {
  return new HostExchange(fn, user, world, compute);
}
GradExchange *kctc_new_cu_probe_exchange(int blocks, double usec, hipStream_t compute) {
  return new CuProbeExchange(blocks, usec, compute);
}

extern "C" {

int kctc_dp_unique_id(void *uid128) {
  return kctc_guarded([&] {
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) throw std::runtime_error("ncclGetUniqueId failed");
    static_assert(sizeof(id) == 128, "ncclUniqueId is 128 bytes");
    memcpy(uid128, &id, sizeof(id));
  });
}

}  // extern "C"
