// ctc_updater.cpp -- NnetCtcUpdater of nnet.h (src/ctc/ctc-nnet-update.cc:76-348)
// and the edit distance of its accuracy.
#include <algorithm>

#include "component_util.h"
#include "ctc.h"

namespace kctc {
namespace nnet2 {

// Unit-cost Levenshtein distance (kaldi::LevenshteinEditDistance,
// src/util/edit-distance-inl.h) by Myers' bit-vector algorithm in its block
// form (Myers 1999; the per-block step as in edlib): column j of the DP over
// ref (rows, 64 per word) is kept as vertical +1/-1 delta masks; one pass per
// hyp symbol costs ceil(m/64) word steps instead of m cell updates.  The
// horizontal delta at the top boundary is +1 (D[0][j] = j); bits above row
// m-1 in the last word never reach lower rows (carries and shifts go up).
int levenshtein(const int *ref, int m, const int *hyp, int n) {
  if (m <= 0) return n > 0 ? n : 0;
  if (n <= 0) return m;
  const int W = (m + 63) / 64;
  int lo = ref[0], hi = ref[0];
  for (int i = 1; i < m; i++) { lo = std::min(lo, ref[i]); hi = std::max(hi, ref[i]); }
  std::vector<uint64_t> peq((size_t)(hi - lo + 2) * W, 0);  // last row: symbols absent from ref
  for (int i = 0; i < m; i++) peq[(size_t)(ref[i] - lo) * W + i / 64] |= 1ull << (i % 64);
  std::vector<uint64_t> P(W, ~0ull), M(W, 0ull);
  const uint64_t last = 1ull << ((m - 1) % 64);
  int score = m;
  for (int j = 0; j < n; j++) {
    const int c = hyp[j];
    const uint64_t *eq = &peq[(size_t)((c >= lo && c <= hi) ? c - lo : hi - lo + 1) * W];
    int hin = 1;
    for (int b = 0; b < W; b++) {
      const uint64_t Pv = P[b], Mv = M[b], hneg = hin < 0 ? 1ull : 0ull;
      uint64_t Eq = eq[b];
      const uint64_t Xv = Eq | Mv;
      Eq |= hneg;
      const uint64_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
      uint64_t Ph = Mv | ~(Xh | Pv);
      uint64_t Mh = Pv & Xh;
      const uint64_t hb = b == W - 1 ? last : (1ull << 63);
      const int hout = (Ph & hb) ? 1 : ((Mh & hb) ? -1 : 0);
      Ph = (Ph << 1) | (hin > 0 ? 1ull : 0ull);
      Mh = (Mh << 1) | hneg;
      P[b] = Mh | ~(Xv | Ph);
      M[b] = Ph & Xv;
      hin = hout;
    }
    score += hin;
  }
  return score;
}

// ---------------------------------------------------------------------------
// NnetCtcUpdater (src/ctc/ctc-nnet-update.cc:76-348)
// ---------------------------------------------------------------------------
NnetCtcUpdater::NnetCtcUpdater(Nnet *nnet, bool update) : nnet_(nnet), update_(update) {}

void NnetCtcUpdater::ComponentsChanged() {
  if (pending_) throw std::logic_error("the component list changed with queued minibatches (Finish them first)");
  // indexed by component: rebuilt by the next minibatch (Output() is empty until then)
  forward_data_.clear();
  chunk_info_.clear();
}

void NnetCtcUpdater::BeginStep(const float *feats, int T_max, int N) {
  if (N <= 0 || T_max <= 0) throw std::invalid_argument("empty minibatch");
  const int C = nnet_->NumComponents();
  nnet_->SetMiniBatch(N);
  // one error word per step for every recurrence: cleared here (stream order:
  // after the previous step's readback), read back at the end, and the
  // updates of a step that set it are skipped on the device
  err_word_.ensure(256);
  KCTC_HIP_CHECK(hipMemsetAsync(err_word_.p, 0, sizeof(unsigned), S()));
  for (int c = 0; c < C; c++)
    if (auto *r = dynamic_cast<CuDNNRecurrentComponent *>(&nnet_->GetComponent(c)))
      r->SetErrorWord(static_cast<unsigned *>(err_word_.p));
  forward_data_.resize(C + 1);
  SetupChunks(T_max, N);
  forward_data_[0].SetView(const_cast<float *>(feats), (long)T_max * N * nnet_->NumSplice(), nnet_->InputDim());
}

void NnetCtcUpdater::ThrowIfErrWord() {
  unsigned herr = 0;
  KCTC_HIP_CHECK(hipMemcpyAsync(&herr, err_word_.p, sizeof(unsigned), hipMemcpyDeviceToHost, S()));
  KCTC_HIP_CHECK(hipStreamSynchronize(S()));
  if (herr) throw std::runtime_error("recurrence hand-off timed out (device error word set)");
}

MinibatchStats NnetCtcUpdater::ComputeForMinibatch(const float *feats, int T_max, int N,
                                                   const int *num_frames, const int *flat_labels,
                                                   const int *label_lengths) {
  if (pending_) throw std::logic_error("ComputeForMinibatch with queued minibatches (Finish them first)");
  Enqueue(feats, T_max, N, num_frames, flat_labels, label_lengths);
  return Finish();
}

const CuMatrixBase &NnetCtcUpdater::Forward(const float *feats, int T_max, int N) {
  if (pending_) throw std::logic_error("Forward with queued minibatches (Finish them first)");
  BeginStep(feats, T_max, N);
  Propagate(T_max, N);
  ThrowIfErrWord();
  return forward_data_.back();
}

const CuMatrixBase &NnetCtcUpdater::ForwardSeq(const float *feats, int T_max, int N, const int *num_frames) {
  if (pending_) throw std::logic_error("ForwardSeq with queued minibatches (Finish them first)");
  // the lengths are checked before anything is set up (BeginStep repeats the shape check)
  if (N <= 0 || T_max <= 0 || !num_frames) throw std::invalid_argument("empty minibatch");
  for (int n = 0; n < N; n++)
    if (num_frames[n] < 1 || num_frames[n] > T_max)
      throw std::invalid_argument("ForwardSeq: num_frames[" + std::to_string(n) + "] = " +
                                  std::to_string(num_frames[n]) + " outside [1, T_max]");
  BeginStep(feats, T_max, N);
  PropagateSeq(T_max, N, num_frames, false);
  ThrowIfErrWord();
  return forward_data_.back();
}

void NnetCtcUpdater::PropagateSeq(int T_max, int N, const int *num_frames, bool train) {
  const int C = nnet_->NumComponents();
  for (int c = 0; c < C; c++) {
    const Component &comp = nnet_->GetComponent(c);
    const CuMatrixBase &in = forward_data_[c];
    CuMatrix &out = forward_data_[c + 1];
    if (comp.IsIdentityForward()) {
      out.SetView(in.Data(), in.NumRows(), comp.OutputDim());
      continue;
    }
    out.Resize((long)T_max * N, comp.OutputDim());
    if (const auto *r = dynamic_cast<const CuDNNRecurrentComponent *>(&comp)) {
      // no streamed hand-over between RNNs here: it reads un-shifted images
      r->ClearPackedInput();
      if (train) {
        r->ClearInputBound();  // (a bound a chained forward once installed: found again by the weight GEMMs' max pass)
        r->PropagateSeqTrain(in, &out, num_frames);
      } else {
        r->PropagateSeq(in, &out, num_frames);
      }
    } else {
      comp.Propagate(chunk_info_[c], chunk_info_[c + 1], in, &out);
    }
  }
}

void NnetCtcUpdater::Enqueue(const float *feats, int T_max, int N, const int *num_frames,
                             const int *flat_labels, const int *label_lengths) {
  if (pending_ == 2) throw std::logic_error("two minibatches already queued");
  if (length_aware_) {  // checked before anything is set up
    if (N > 64) throw std::invalid_argument("length-aware minibatches hold at most 64 utterances");
    for (int n = 0; n < N && num_frames; n++)
      if (num_frames[n] < 1 || num_frames[n] > T_max)
        throw std::invalid_argument("length-aware minibatch: num_frames[" + std::to_string(n) + "] = " +
                                    std::to_string(num_frames[n]) + " outside [1, T_max]");
    for (int c = 0; c < nnet_->NumComponents(); c++)
      if (auto *r = dynamic_cast<CuDNNRecurrentComponent *>(&nnet_->GetComponent(c)))
        if (r->Desc().prec != 0)
          throw std::invalid_argument("length-aware minibatches need fp32-class precision (bf16 is set)");
  }
  BeginStep(feats, T_max, N);
  const int C = nnet_->NumComponents();
  const long rows = (long)T_max * N;
  if (inject_err_) {
    KCTC_HIP_CHECK(hipMemcpyAsync(err_word_.p, &inject_err_, sizeof(unsigned), hipMemcpyHostToDevice, S()));
    KCTC_HIP_CHECK(hipStreamSynchronize(S()));  // the source is a member that is reset next
    inject_err_ = 0;
  }
  if (length_aware_) PropagateSeq(T_max, N, num_frames, update_);
  else Propagate(T_max, N);

  // ---- ComputeObjfAndDeriv (:171-259) with the warp-ctc ABI ----
  const CuMatrixBase &out = forward_data_[C];
  const int A = nnet_->OutputDim();
  for (int n = 0; n < N; n++)
    if (label_lengths[n] < 0) throw std::invalid_argument("negative label length");
  // input_lengths = NumFrames - ignore_frames (left_context + RightContext = 0 here)
  size_t ws = 0;
  {
    ctcOptions o;
    o.loc = CTC_GPU;
    o.stream = reinterpret_cast<ctcStream_t>(S());
    o.blank_label = 0;
    ctcStatus_t st = get_workspace_size(label_lengths, num_frames, A, N, o, &ws);
    if (st != CTC_STATUS_SUCCESS)
      throw std::runtime_error(std::string("get_workspace_size: ") + ctcGetStatusString(st));
    // size for the longest labels this T_max admits, once: a growing workspace
    // (label lengths vary per minibatch) would cost a device sync + realloc
    if (ws > ctc_ws_.bytes) {
      std::vector<int> worst_l(N, std::min(T_max, 639)), worst_t(N, T_max);
      size_t w2 = 0;
      if (get_workspace_size(worst_l.data(), worst_t.data(), A, N, o, &w2) == CTC_STATUS_SUCCESS)
        ws = std::max(ws, w2);
    }
  }
  ctc_ws_.ensure(ws);
  costs_dev_.ensure(sizeof(double) * N);
  ids_dev_.ensure(sizeof(int) * rows);
  CuMatrix &deriv = deriv_a_;
  deriv.Resize(rows, A);
  {
    ProfScope ps("layer_ctc");
    ctcStatus_t st = mictc_compute_ctc_loss_async(out.Data(), update_ ? deriv.Data() : nullptr,
                                                  flat_labels, label_lengths, num_frames, A, N,
                                                  static_cast<double *>(costs_dev_.p), ctc_ws_.p,
                                                  reinterpret_cast<ctcStream_t>(S()), 0);
    if (st != CTC_STATUS_SUCCESS)
      throw std::runtime_error(std::string("compute_ctc_loss: ") + ctcGetStatusString(st));
  }
  {
    ProfScope ps("argmax");
    row_argmax(S(), out.Data(), rows, A, static_cast<int *>(ids_dev_.p));  // FindRowMaxId
  }
  if (update_) Backprop(T_max, N);

  // ---- the single end-of-step device->host copy: costs, best-path ids,
  // the RNN components' device error words (into this slot's pinned buffer)
  Slot &sl = slots_[next_];
  const size_t need = sizeof(double) * N + sizeof(int) * rows + sizeof(unsigned) * C;
  if (need > sl.bytes) {
    if (sl.pinned) {
      if (sl.ev) KCTC_HIP_CHECK(hipEventSynchronize(sl.ev));
      (void)hipHostFree(sl.pinned);
    }
    KCTC_HIP_CHECK(hipHostMalloc((void **)&sl.pinned, need, hipHostMallocDefault));
    sl.bytes = need;
  }
  if (!sl.ev) KCTC_HIP_CHECK(hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
  double *hcost = reinterpret_cast<double *>(sl.pinned);
  int *hids = reinterpret_cast<int *>(sl.pinned + sizeof(double) * N);
  unsigned *herr = reinterpret_cast<unsigned *>(hids + rows);
  KCTC_HIP_CHECK(hipMemcpyAsync(hcost, costs_dev_.p, sizeof(double) * N, hipMemcpyDeviceToHost, S()));
  KCTC_HIP_CHECK(hipMemcpyAsync(hids, ids_dev_.p, sizeof(int) * rows, hipMemcpyDeviceToHost, S()));
  sl.nerr = 1;
  KCTC_HIP_CHECK(hipMemcpyAsync(herr, err_word_.p, sizeof(unsigned), hipMemcpyDeviceToHost, S()));
  KCTC_HIP_CHECK(hipEventRecord(sl.ev, S()));
  sl.N = N;
  sl.rows = rows;
  sl.num_frames.assign(num_frames, num_frames + N);
  long nlab = 0;
  for (int n = 0; n < N; n++) nlab += label_lengths[n];
  sl.labels.assign(flat_labels, flat_labels + nlab);
  sl.label_lengths.assign(label_lengths, label_lengths + N);
  next_ ^= 1;
  pending_++;
}

MinibatchStats NnetCtcUpdater::Finish() {
  if (!pending_) throw std::logic_error("no queued minibatch");
  Slot &sl = slots_[next_ ^ (pending_ == 2 ? 0 : 1)];  // the oldest
  pending_--;
  KCTC_HIP_CHECK(hipEventSynchronize(sl.ev));
  if (!pending_) CuDevice::Instantiate().Collect();  // no span of a later minibatch in flight
  const int N = sl.N;
  const long rows = sl.rows;
  const double *hcost = reinterpret_cast<const double *>(sl.pinned);
  const int *hids = reinterpret_cast<const int *>(sl.pinned + sizeof(double) * N);
  const unsigned *herr = reinterpret_cast<const unsigned *>(hids + rows);
  last_ids_.assign(hids, hids + rows);
  last_costs_.assign(hcost, hcost + N);
  for (int i = 0; i < sl.nerr; i++) {
    if (herr[i] & ~kErrPeerFailed) {
      // bits: 1 a recurrence's spin, 2 a streamed GEMM's wait, 8 a weight-gradient gate
      char what[64];
      snprintf(what, sizeof what, " (error word %d = 0x%x)", i, herr[i]);
      throw std::runtime_error(std::string("recurrence hand-off timed out") + what +
                               "; this minibatch's updates were skipped, the parameters are those before it");
    }
    if (herr[i])
      throw std::runtime_error("the step failed on another data-parallel rank; every rank skipped this "
                               "minibatch's updates, the parameters are those before it");
  }
  const int *num_frames = sl.num_frames.data(), *flat_labels = sl.labels.data();
  const int *label_lengths = sl.label_lengths.data();
  MinibatchStats st;
  for (int n = 0; n < N; n++) st.tot_objf += hcost[n];
  if (!(st.tot_objf == st.tot_objf)) throw std::runtime_error("costs sum is nan");  // :254
  // ---- ComputeTotAccuracy (:261-317) on the host ----
  const int blank = 0;
  long off = 0;
  double err = 0;
  std::vector<int> hyp;
  for (int n = 0; n < N; n++) {
    const int F = num_frames[n], L = label_lengths[n];
    hyp.assign((size_t)std::max(F, 0), 0);
    for (int i = 0; i < F; i++) hyp[i] = hids[(long)i * N + n];
    int i = 1, j = 1;
    while (j < F) {
      if (hyp[j] != hyp[j - 1] && hyp[j] != blank) hyp[i++] = hyp[j];
      j++;
    }
    hyp.resize(F > 0 ? i : 0);
    // LevenshteinEditDistance, unit costs
    err += levenshtein(flat_labels + off, L, hyp.data(), (int)hyp.size());
    st.tot_weight += L;
    off += L;
  }
  st.tot_accuracy = st.tot_weight - err;
  return st;
}

// Nnet::ComputeChunkInfo(num_splice, T*N) (nnet-nnet.cc:75-133) for the
// contiguous case: the last component's output is frame offset L (the
// network's left context), every component's input starts Context().front()
// frames earlier.  Rows: T*N*num_splice before a splicing component (the
// FormatNnetInput layout, ctc-nnet-update.cc:351-424), T*N after it; such a
// component must come first (the nnet2 CTC recipe's Splice).
void NnetCtcUpdater::SetupChunks(int T_max, int N) {
  const int C = nnet_->NumComponents();
  chunk_info_.resize(C + 1);
  int off = nnet_->LeftContext();
  for (int c = C; c >= 0; c--) {
    chunk_info_[c].num_chunks = N;
    chunk_info_[c].chunk_size = T_max;
    chunk_info_[c].feat_dim = c == 0 ? nnet_->InputDim() : nnet_->GetComponent(c - 1).OutputDim();
    chunk_info_[c].first_offset = off;
    if (c > 0) {
      const std::vector<int> ctx = nnet_->GetComponent(c - 1).Context();
      if (c - 1 > 0 && ctx != std::vector<int>{0})
        throw std::invalid_argument("a component with context other than {0} must come first (the recipe's Splice)");
      off += ctx.front();
    }
  }
}

void NnetCtcUpdater::Propagate(int T, int N) {  // :136-169
  const int C = nnet_->NumComponents();
  const CuDNNRecurrentComponent *below = nullptr;  // the last RNN, through identity components
  const int first = nnet_->FirstUpdatableComponent();
  for (int c = 0; c < C; c++) {
    const Component &comp = nnet_->GetComponent(c);
    if (const auto *r = dynamic_cast<const CuDNNRecurrentComponent *>(&comp)) {
      const void *rows = nullptr, *cols = nullptr;
      if (below && below->Desc().prec == r->Desc().prec) below->PackedOutput(&rows, &cols);
      r->SetPackedInput(rows, cols);
      if (!below) r->ClearInputBound();  // e.g. above a DropoutComponent: |input| can exceed 1
      // Backprop computes its input derivative (streamed dx GEMM): W^T packed now
      r->SetPrepackDx(update_ && c > first);
      r->SetPrepackW(update_ && c >= first);
      below = r;
    } else if (!comp.IsIdentityForward()) {
      below = nullptr;
    }
    const CuMatrixBase &in = forward_data_[c];
    CuMatrix &out = forward_data_[c + 1];
    if (comp.IsIdentityForward()) {
      out.SetView(in.Data(), in.NumRows(), comp.OutputDim());  // alias, no copy
      continue;
    }
    out.Resize((long)T * N, comp.OutputDim());
    // RNN -> identity-forward components -> RNN: the second one's input
    // projection streams off the first one's last recurrence
    const auto *rnn = dynamic_cast<const CuDNNRecurrentComponent *>(&comp);
    const CuDNNRecurrentComponent *next = nullptr;
    if (rnn) {
      int c2 = c + 1;
      while (c2 < C && nnet_->GetComponent(c2).IsIdentityForward()) c2++;
      if (c2 < C) next = dynamic_cast<const CuDNNRecurrentComponent *>(&nnet_->GetComponent(c2));
    }
    if (next) rnn->PropagateChained(in, &out, *next);
    else comp.Propagate(chunk_info_[c], chunk_info_[c + 1], in, &out);
  }
}

void NnetCtcUpdater::Backprop(int T, int N) {  // :320-348
  const int C = nnet_->NumComponents();
  const long rows = (long)T * N;
  const int A = nnet_->OutputDim();
  // deriv->Scale(-1) (:323)
  {
    ProfScope ps("scale");
    scale_inplace(S(), deriv_a_.Data(), rows * (long)A, -1.f);
  }
  CuMatrix *cur = &deriv_a_, *other = &deriv_b_;
  const int first = nnet_->FirstUpdatableComponent();
  int max_dim = A;
  for (int c = 0; c <= C; c++) max_dim = std::max(max_dim, chunk_info_[c].feat_dim);
  std::vector<int> updated;
  for (int c = C - 1; c >= first; c--) {
    Component &comp = nnet_->GetComponent(c);
    const CuMatrixBase &in = forward_data_[c], &outv = forward_data_[c + 1];
    Component *to_update = &comp;
    const bool need_in_deriv = c > first;
    CuMatrixBase *in_deriv = nullptr;
    CuMatrixBase view;
    if (need_in_deriv) {
      if (comp.IsIdentityForward()) {
        view = CuMatrixBase(cur->Data(), rows, comp.InputDim());  // in place
        in_deriv = &view;
      } else {
        other->Resize(rows, std::max(comp.InputDim(), max_dim));
        view = CuMatrixBase(other->Data(), rows, comp.InputDim());
        in_deriv = &view;
      }
    }
    if (auto *cg = dynamic_cast<ClipGradientComponent *>(&comp)) {
      cg->rng_ = &repair_rng_;  // RepairGradients draws RandUniform() from the process stream
      if (cg->Shadow()) to_update = cg->Shadow();  // momentum: delta_nnet's copy
    }
    if (auto *rl = dynamic_cast<RectifiedLinearComponent *>(&comp))
      if (rl->Shadow()) to_update = rl->Shadow();  // ditto: UpdateStats goes to the delta copy
    const CuMatrixBase od(cur->Data(), rows, comp.OutputDim());
    const bool rec = exchange_ && dynamic_cast<CuDNNRecurrentComponent *>(&comp);
    if (rec) exchange_->BeforeRecurrence(S());
    comp.Backprop(chunk_info_[c], chunk_info_[c + 1], in, outv, od, to_update, in_deriv);
    if (rec) exchange_->AfterRecurrence();
    if (comp.IsUpdatable()) {
      auto *u = static_cast<UpdatableComponent *>(&comp);
      if (exchange_) exchange_->GradReady(c, u->GradData(), u->NumParameters(), u->GradStream());
      updated.push_back(c);
    }
    if (need_in_deriv && !comp.IsIdentityForward()) std::swap(cur, other);
  }
  CuDevice::Instantiate().Join();
  if (exchange_) exchange_->Finish();
  if (exchange_ && exchange_->WorldSize() > 1 && err_word_.p) {
    // the gradients just summed include every rank's: a step that failed on
    // ANY rank is skipped on all of them, so the replicas stay identical
    unsigned *err = static_cast<unsigned *>(err_word_.p);
    err_flag_.ensure(256);
    err_word_to_flag(S(), err, err_flag_.f());
    exchange_->AllReduceSum(err_flag_.f(), 1, S());
    flag_to_err_word(S(), err_flag_.f(), err);
  }
  for (int c : updated) {
    ProfScope ps("update");
    static_cast<UpdatableComponent *>(&nnet_->GetComponent(c))->ApplyUpdate(err_word_.p ? static_cast<const unsigned *>(err_word_.p) : nullptr);
  }
  // momentum: nnet->AddNnet(1.0, *delta_nnet); delta_nnet->Scale(momentum) on the
  // NonlinearComponent statistics (the parameters' share is ApplyUpdate's).
  // Not gated by the step's error word: like ClipGradient's counters the
  // statistics count every minibatch whose Backprop ran, also one whose
  // parameter updates are skipped.
  if (nnet_->Momentum() != 0.f)
    for (int c = first; c < C; c++)
      if (auto *rl = dynamic_cast<RectifiedLinearComponent *>(&nnet_->GetComponent(c))) rl->FoldShadow(nnet_->Momentum());
}

}  // namespace nnet2
}  // namespace kctc
