// rnn_component.cpp -- CuDNNRecurrentComponent of nnet.h
// (nnet-cudnn-component.cc:56-772) on the recurrences of rnn.h.
#include "component_util.h"

namespace kctc {
namespace nnet2 {

CuDNNRecurrentComponent::CuDNNRecurrentComponent() {
  desc_.mode = kLstm;
  desc_.dirs = 2;
  KCTC_HIP_CHECK(hipMalloc(&err_, 256));
  KCTC_HIP_CHECK(hipMemset(err_, 0, 256));
}
CuDNNRecurrentComponent::~CuDNNRecurrentComponent() {
  if (err_) (void)hipFree(err_);
  if (pre_.ev) (void)hipEventDestroy(pre_.ev);
  if (pre_.wev) (void)hipEventDestroy(pre_.wev);
}

void CuDNNRecurrentComponent::InitFromString(std::string args, Rng &rng) {
  const std::string orig = args;
  bool ok = true, bidir = true;
  int layers = 0, D = 0, H = 0, mode = 2, mb = 0;
  ok = ok && ParseFromString("learning-rate", &args, &learning_rate_);
  ok = ok && ParseFromString("num-layers", &args, &layers);
  ok = ok && ParseFromString("input-dim", &args, &D);
  ok = ok && ParseFromString("output-dim", &args, &H);
  ok = ok && ParseFromString("rnn-mode", &args, &mode);
  ok = ok && ParseFromString("bidirectional", &args, &bidir);
  ok = ok && ParseFromString("max-seq-length", &args, &max_seq_length_);
  ParseFromString("param-stddev", &args, &param_stddev_);
  ParseFromString("bias-stddev", &args, &bias_stddev_);
  ParseFromString("clip-gradient", &args, &clip_gradient_);
  ParseFromString("mini-batch", &args, &mb);
  if (!ok) throw std::invalid_argument("Bad initializer " + orig);
  if (mode < 0 || mode > 3)
    throw std::invalid_argument("rnn_mode_ = " + std::to_string(mode) + ", should in [0, 1, 2, 3].");
  desc_.mode = mode;
  desc_.D = D;
  desc_.H = H;
  desc_.layers = layers;
  desc_.dirs = bidir ? 2 : 1;
  Init(rng);
}

// weights: every lin-layer matrix ~ N(0, param_stddev^2), every bias vector =
// bias_stddev (SetRandn then Set, nnet-cudnn-component.cc:336-407)
void CuDNNRecurrentComponent::Init(Rng &rng) {
  const long P = desc_.params_size();
  std::vector<float> h((size_t)P, 0.f);
  const int nlin = 2 * desc_.nw();
  for (int pl = 0; pl < desc_.layers * desc_.dirs; pl++) {
    for (int lin = 0; lin < nlin; lin++) {
      const long off = desc_.lin_offset(pl, lin, false);
      const long n = (long)desc_.H * (lin < desc_.nw() ? desc_.din(pl / desc_.dirs) : desc_.H);
      for (long i = 0; i < n; i++) h[off + i] = (float)(rng.gauss() * param_stddev_);
      const long bo = desc_.lin_offset(pl, lin, true);
      for (long i = 0; i < desc_.H; i++) h[bo + i] = bias_stddev_;
    }
  }
  params_.ensure(sizeof(float) * P);
  grad_.ensure(sizeof(float) * P);
  h2d(params_.f(), h.data(), P);
}

std::string CuDNNRecurrentComponent::Info() const {
  std::ostringstream os;
  os << Type() << ", input-dim=" << desc_.D << ", output-dim=" << OutputDim()
     << ", learning-rate=" << learning_rate_ << ", hidden-dim=" << desc_.H
     << ", num-layers=" << desc_.layers << ", max-seq-length=" << max_seq_length_
     << ", rnn-mode=" << desc_.mode << (desc_.dirs == 2 ? ", BIDIRECTIONAL" : ", UNIDIRECTIONAL");
  return os.str();
}

void CuDNNRecurrentComponent::Propagate(const ChunkInfo &, const ChunkInfo &, const CuMatrixBase &in,
                                        CuMatrixBase *out) const {
  Forward(in, out, nullptr);
}

void CuDNNRecurrentComponent::PropagateChained(const CuMatrixBase &in, CuMatrixBase *out,
                                               const CuDNNRecurrentComponent &next) const {
  auto &dev = CuDevice::Instantiate();
  const int N = mini_batch_ > 0 ? mini_batch_ : 1;
  const int T = (int)(in.NumRows() / N);
  // |h| <= 1 for LSTM / GRU / TANH outputs: the next RNN's input needs no max pass
  next.input_bound_ = desc_.mode != kRelu ? 1.f : 0.f;
  if (!dev.side || next.mini_batch_ != N || next.desc_.D != OutputDim()) {
    Forward(in, out, nullptr);
    return;
  }
  next.reserve_.ensure(sizeof(float) * rnn_reserve_layout(next.desc_, T, N).total);
  next.workspace_.ensure(rnn_workspace_bytes(next.desc_, T, N));
  RnnFwdChain c;
  c.d = &next.desc_; c.w = next.params_.f();
  c.workspace = next.workspace_.p; c.ws_bytes = next.workspace_.bytes;
  c.reserve = next.reserve_.p; c.res_bytes = next.reserve_.bytes;
  c.side = dev.side;
  Forward(in, out, &c);
  next.input_projected_ = c.done;
}

void CuDNNRecurrentComponent::Forward(const CuMatrixBase &in, CuMatrixBase *out, RnnFwdChain *chain) const {
  // seq_length = rows / mini_batch, no masking (nnet-cudnn-component.cc:521-555)
  const int N = mini_batch_ > 0 ? mini_batch_ : 1;
  const int T = (int)(in.NumRows() / N);
  if (in.NumCols() != desc_.D || in.NumRows() % N)
    throw std::invalid_argument("CuDNNRecurrentComponent::Propagate: bad input shape");
  seq_length_ = T;
  seq_lens_.clear();
  reserve_.ensure(sizeof(float) * rnn_reserve_layout(desc_, T, N).total);
  workspace_.ensure(rnn_workspace_bytes(desc_, T, N));
  const bool projected = input_projected_;
  input_projected_ = false;
  in_tn_[0] = T;
  in_tn_[1] = N;
  ProfScope ps("layer_rnn_forward");
  // the trainer's side stream (idle during the forward pass): the W^T / x^T /
  // y^T prepacks beside the recurrence (rnn.h RnnPrepack)
  auto &dev = CuDevice::Instantiate();
  hipStream_t side = S() == dev.stream ? dev.side : nullptr;
  RnnPrepack *pre = nullptr;
  if ((prepack_dx_ || prepack_w_) && side) {
    if (!pre_.ev) KCTC_HIP_CHECK(hipEventCreateWithFlags(&pre_.ev, hipEventDisableTiming));
    if (!pre_.wev) KCTC_HIP_CHECK(hipEventCreateWithFlags(&pre_.wev, hipEventDisableTiming));
    // the dx-stream queue (idle in the forward pass): the side stream carries
    // the next component's projection streamed off this recurrence
    pre_.stream = dev.stream2 ? dev.stream2 : side;
    pre_.dx = prepack_dx_;
    pre_.wgrad = prepack_w_;
    pre_.in_bound = input_bound_;
    pre = &pre_;
  }
  pre_.done = pre_.wdone = false;
  pre_x_ = in.Data();
  pre_y_ = out->Data();
  RnnFwdOpts o;
  o.chain = chain; o.input_projected = projected; o.in_rows = in_rows_; o.pre = pre;
  int st = rnn_forward_training(desc_, S(), T, N, in.Data(), params_.f(), out->Data(), workspace_.p,
                                workspace_.bytes, reserve_.p, reserve_.bytes, DeviceError(), o);
  pre_ver_ = pver_;
  if (st) throw std::runtime_error("rnn_forward_training failed: " + std::to_string(st));
}

void CuDNNRecurrentComponent::PropagateSeq(const CuMatrixBase &in, CuMatrixBase *out, const int *num_frames) const {
  const int N = mini_batch_ > 0 ? mini_batch_ : 1;
  const int T = (int)(in.NumRows() / N);
  if (in.NumCols() != desc_.D || in.NumRows() % N || !num_frames)
    throw std::invalid_argument("CuDNNRecurrentComponent::PropagateSeq: bad input shape");
  reserve_.ensure(sizeof(float) * rnn_reserve_layout(desc_, T, N).total);
  workspace_.ensure(rnn_workspace_bytes(desc_, T, N));
  seq_buf_.ensure(rnn_seq_buffer_bytes(desc_, T, N));
  // the reserve no longer holds a training forward, and nothing was streamed
  seq_length_ = 0;
  seq_lens_.clear();
  input_projected_ = false;
  in_tn_[0] = in_tn_[1] = -1;
  pre_.done = pre_.wdone = false;
  ProfScope ps("layer_rnn_forward");
  int st = rnn_forward_inference_seq(desc_, S(), T, N, num_frames, in.Data(), params_.f(), out->Data(), workspace_.p,
                                     workspace_.bytes, reserve_.p, reserve_.bytes, seq_buf_.p, seq_buf_.bytes,
                                     DeviceError());
  if (st) throw std::runtime_error("rnn_forward_inference_seq failed: " + std::to_string(st));
}

void CuDNNRecurrentComponent::PropagateSeqTrain(const CuMatrixBase &in, CuMatrixBase *out,
                                                const int *num_frames) const {
  const int N = mini_batch_ > 0 ? mini_batch_ : 1;
  const int T = (int)(in.NumRows() / N);
  if (in.NumCols() != desc_.D || in.NumRows() % N || !num_frames)
    throw std::invalid_argument("CuDNNRecurrentComponent::PropagateSeqTrain: bad input shape");
  reserve_.ensure(rnn_seq_train_reserve_bytes(desc_, T, N));
  workspace_.ensure(rnn_seq_train_workspace_bytes(desc_, T, N));
  // the reserve holds a length-aware training forward; nothing was streamed or prepacked
  seq_length_ = T;
  seq_lens_.assign(num_frames, num_frames + N);
  input_projected_ = false;
  in_tn_[0] = in_tn_[1] = -1;
  pre_.done = pre_.wdone = false;
  ProfScope ps("layer_rnn_forward");
  int st = rnn_forward_training_seq(desc_, S(), T, N, num_frames, in.Data(), params_.f(), out->Data(), workspace_.p,
                                    workspace_.bytes, reserve_.p, reserve_.bytes, DeviceError());
  if (st) {
    seq_lens_.clear();
    throw std::runtime_error("rnn_forward_training_seq failed: " + std::to_string(st));
  }
}

void CuDNNRecurrentComponent::BackpropSeq(const CuMatrixBase &in_value, const CuMatrixBase &out_value,
                                          const CuMatrixBase &out_deriv, Component *to_update_in,
                                          CuMatrixBase *in_deriv) const {
  const int N = mini_batch_, T = seq_length_;
  if ((int)seq_lens_.size() != N) throw std::logic_error("CuDNNRecurrentComponent: Backprop after another minibatch");
  {
    ProfScope ps("layer_rnn_backward_data");
    int st = rnn_backward_data_seq(desc_, S(), T, N, seq_lens_.data(), out_value.Data(), out_deriv.Data(),
                                   params_.f(), in_deriv ? in_deriv->Data() : nullptr, workspace_.p, workspace_.bytes,
                                   reserve_.p, reserve_.bytes, DeviceError());
    if (st) throw std::runtime_error("rnn_backward_data_seq failed: " + std::to_string(st));
  }
  if (!to_update_in) return;
  auto *to_update = dynamic_cast<CuDNNRecurrentComponent *>(to_update_in);
  if (!to_update) throw std::invalid_argument("CuDNNRecurrentComponent: bad to_update");
  // as Backprop: on the side stream beside the next component's backward recurrence
  auto &dev = CuDevice::Instantiate();
  hipStream_t ws = dev.side ? dev.side : S();
  dev.Fork();
  to_update->grad_stream_ = ws;
  KCTC_HIP_CHECK(hipMemsetAsync(to_update->grad_.p, 0, sizeof(float) * NumParameters(), ws));
  ProfScope ps("layer_rnn_backward_weights", ws);
  RnnWgradOpts o;
  o.max_blocks = dev.side ? side_gemm_blocks() : 0; o.in_bound = input_bound_;
  o.s2 = (!in_deriv && dev.side) ? dev.stream2 : nullptr;
  o.beside = in_deriv && dev.side;
  int st = rnn_backward_weights_seq(desc_, ws, T, N, seq_lens_.data(), in_value.Data(), out_value.Data(),
                                    workspace_.p, workspace_.bytes, to_update->grad_.f(), reserve_.p, reserve_.bytes,
                                    o);
  if (st) throw std::runtime_error("rnn_backward_weights_seq failed: " + std::to_string(st));
}

void CuDNNRecurrentComponent::Backprop(const ChunkInfo &, const ChunkInfo &,
                                       const CuMatrixBase &in_value, const CuMatrixBase &out_value,
                                       const CuMatrixBase &out_deriv, Component *to_update_in,
                                       CuMatrixBase *in_deriv) const {
  if (!seq_lens_.empty()) return BackpropSeq(in_value, out_value, out_deriv, to_update_in, in_deriv);
  const int N = mini_batch_, T = seq_length_;
  auto &dev0 = CuDevice::Instantiate();
  // the bottom component (no input derivative): its weight gradients are
  // streamed off its own backward recurrence on the side stream (rnn.h
  // RnnWgradStream) instead of following it
  if (to_update_in && !in_deriv && dev0.side && rnn_wgrad_stream_ok(desc_, T, N)) {
    auto *to_update = dynamic_cast<CuDNNRecurrentComponent *>(to_update_in);
    if (!to_update) throw std::invalid_argument("CuDNNRecurrentComponent: bad to_update");
    hipStream_t ws = dev0.side;
    dev0.Fork();
    to_update->grad_stream_ = ws;
    KCTC_HIP_CHECK(hipMemsetAsync(to_update->grad_.p, 0, sizeof(float) * NumParameters(), ws));
    RnnWgradStream wg;
    wg.side = ws;
    if (const char *e = getenv("KCTC_WGRAD_CHUNKS")) wg.chunks = atoi(e);
    wg.x = in_value.Data();
    wg.dw = to_update->grad_.f();
    wg.max_blocks = side_gemm_blocks();
    wg.in_bound = input_bound_;
    {
      ProfScope ps("layer_rnn_backward_data");
      int st = rnn_backward_data(desc_, S(), T, N, out_value.Data(), out_deriv.Data(), params_.f(), nullptr,
                                 workspace_.p, workspace_.bytes, reserve_.p, reserve_.bytes, DeviceError(),
                                 dev0.stream2, &wg);
      if (st) throw std::runtime_error("rnn_backward_data failed: " + std::to_string(st));
    }
    if (!wg.done) {
      dev0.Fork();
      ProfScope ps("layer_rnn_backward_weights", ws);
      RnnWgradOpts o;
      o.max_blocks = side_gemm_blocks(); o.in_bound = input_bound_;
      o.in_cols = packed_input_cols(T, N); o.pre = wgrad_prepack(in_value, out_value);
      int st = rnn_backward_weights(desc_, ws, T, N, in_value.Data(), out_value.Data(), workspace_.p,
                                    workspace_.bytes, to_update->grad_.f(), reserve_.p, reserve_.bytes, o);
      if (st) throw std::runtime_error("rnn_backward_weights failed: " + std::to_string(st));
    }
    return;
  }
  {
    ProfScope ps("layer_rnn_backward_data");
    // the forward's packed W^T, if the parameters are still the ones it packed
    const RnnPrepack *pre = pre_.done && pre_ver_ == pver_ ? &pre_ : nullptr;
    int st = rnn_backward_data(desc_, S(), T, N, out_value.Data(), out_deriv.Data(), params_.f(),
                               in_deriv ? in_deriv->Data() : nullptr, workspace_.p, workspace_.bytes,
                               reserve_.p, reserve_.bytes, DeviceError(), CuDevice::Instantiate().stream2, nullptr,
                               pre);
    if (st) throw std::runtime_error("rnn_backward_data failed: " + std::to_string(st));
  }
  if (to_update_in) {
    auto *to_update = dynamic_cast<CuDNNRecurrentComponent *>(to_update_in);
    if (!to_update) throw std::invalid_argument("CuDNNRecurrentComponent: bad to_update");
    // filter_params_grad_ is zeroed, then cudnnRNNBackwardWeights accumulates.
    // On the side stream (when there is one) so the weight GEMMs overlap the
    // next component's backward recurrence; only this component's reserve,
    // workspace and gradient are touched there.
    auto &dev = CuDevice::Instantiate();
    hipStream_t ws = dev.side ? dev.side : S();
    dev.Fork();
    to_update->grad_stream_ = ws;
    KCTC_HIP_CHECK(hipMemsetAsync(to_update->grad_.p, 0, sizeof(float) * NumParameters(), ws));
    ProfScope ps("layer_rnn_backward_weights", ws);
    RnnWgradOpts o;
    o.max_blocks = dev.side ? side_gemm_blocks() : 0; o.in_bound = input_bound_;
    // the bottom component (no input derivative): its weight GEMMs are the
    // step's tail, so dW runs beside dR on the (then idle) dx-stream queue
    o.s2 = (!in_deriv && dev.side) ? dev.stream2 : nullptr;
    o.in_cols = packed_input_cols(T, N); o.pre = wgrad_prepack(in_value, out_value);
    o.beside = in_deriv && dev.side;  // the next component's backward runs beside
    int st = rnn_backward_weights(desc_, ws, T, N, in_value.Data(), out_value.Data(), workspace_.p,
                                  workspace_.bytes, to_update->grad_.f(), reserve_.p, reserve_.bytes, o);
    if (st) throw std::runtime_error("rnn_backward_weights failed: " + std::to_string(st));
  }
}

// x^T / y^T packed by the last forward, if this backward is for that forward's data
const RnnPrepack *CuDNNRecurrentComponent::wgrad_prepack(const CuMatrixBase &in_value,
                                                         const CuMatrixBase &out_value) const {
  return pre_.wdone && in_value.Data() == pre_x_ && out_value.Data() == pre_y_ ? &pre_ : nullptr;
}

bool CuDNNRecurrentComponent::PackedOutput(const void **rows, const void **cols) const {
  *rows = *cols = nullptr;
  if (!reserve_.p || seq_length_ <= 0 || mini_batch_ <= 0) return false;
  if (reserve_.bytes < sizeof(float) * (size_t)rnn_reserve_layout(desc_, seq_length_, mini_batch_).total) return false;
  return rnn_packed_output(desc_, seq_length_, mini_batch_, reserve_.p, rows, cols);
}

int CuDNNRecurrentComponent::side_gemm_blocks() const {
  return 512;  // dynamic tile scheduling: two per CU, late starters exit
}

void CuDNNRecurrentComponent::ApplyUpdate(const unsigned *skip) {
  // ApplyFloor(-clip) / ApplyCeiling(clip) then filter_params_ += lr * grad
  ++pver_;
  UpdateWith(params_.f(), grad_.f(), clip_gradient_, skip);
}

// CuDNNRecurrentComponent(const CuDNNRecurrentComponent &) (nnet-cudnn-component.cc:650-671):
// configuration and filter_params_, no minibatch state (mini_batch_ = 0)
Component *CuDNNRecurrentComponent::Copy() const {
  auto *c = new CuDNNRecurrentComponent;
  c->CopyUpdatableFrom(*this);
  c->desc_ = desc_;
  c->max_seq_length_ = max_seq_length_;
  c->param_stddev_ = param_stddev_;
  c->bias_stddev_ = bias_stddev_;
  c->clip_gradient_ = clip_gradient_;
  const long P = NumParameters();
  c->params_.ensure(sizeof(float) * P);
  c->grad_.ensure(sizeof(float) * P);
  KCTC_HIP_CHECK(hipMemcpyAsync(c->params_.p, params_.p, sizeof(float) * P, hipMemcpyDeviceToDevice, S()));
  return c;
}

// :723-730 (SetBufferZero: the reserve is rebuilt by the next Propagate here)
void CuDNNRecurrentComponent::SetZero(bool treat_as_gradient) {
  UpdatableComponent::SetZero(treat_as_gradient);
  input_projected_ = false;
}

void CuDNNRecurrentComponent::Vectorize(float *host) const {
  auto v = d2h(params_.f(), NumParameters());
  std::copy(v.begin(), v.end(), host);
}
void CuDNNRecurrentComponent::UnVectorize(const float *host) {
  ++pver_;
  h2d(params_.f(), host, NumParameters());
}

// nnet-cudnn-component.cc:698-721
void CuDNNRecurrentComponent::Write(std::ostream &os, bool binary) const {
  WriteToken(os, binary, "<CuDNNRecurrentComponent>");
  WriteToken(os, binary, "<LearningRate>");
  kio::WriteFloat(os, binary, learning_rate_);
  WriteToken(os, binary, "<IsGradient>");
  kio::WriteBool(os, binary, is_gradient_);
  WriteToken(os, binary, "<ClipGradient>");
  kio::WriteFloat(os, binary, clip_gradient_);
  WriteToken(os, binary, "<InputDim>");
  kio::WriteInt(os, binary, desc_.D);
  WriteToken(os, binary, "<HiddenDim>");
  kio::WriteInt(os, binary, desc_.H);
  WriteToken(os, binary, "<NumLayers>");
  kio::WriteInt(os, binary, desc_.layers);
  WriteToken(os, binary, "<Bidirectional>");
  kio::WriteBool(os, binary, desc_.dirs == 2);
  WriteToken(os, binary, "<RNNMode>");
  kio::WriteInt(os, binary, desc_.mode);
  WriteToken(os, binary, "<MaxSeqLength>");
  kio::WriteInt(os, binary, max_seq_length_);
  WriteToken(os, binary, "<FilterParams>");
  auto v = d2h(params_.f(), NumParameters());
  kio::WriteFloatVector(os, binary, v.data(), (long)v.size());
  WriteToken(os, binary, "</CuDNNRecurrentComponent>");
}// nnet-cudnn-component.cc:673-696
void CuDNNRecurrentComponent::Read(std::istream &is, bool binary) {
  ExpectToken(is, binary, "<LearningRate>");
  learning_rate_ = kio::ReadFloat(is, binary);
  ExpectToken(is, binary, "<IsGradient>");
  is_gradient_ = kio::ReadBool(is, binary);
  ExpectToken(is, binary, "<ClipGradient>");
  clip_gradient_ = kio::ReadFloat(is, binary);
  ExpectToken(is, binary, "<InputDim>");
  desc_.D = kio::ReadInt(is, binary);
  ExpectToken(is, binary, "<HiddenDim>");
  desc_.H = kio::ReadInt(is, binary);
  ExpectToken(is, binary, "<NumLayers>");
  desc_.layers = kio::ReadInt(is, binary);
  ExpectToken(is, binary, "<Bidirectional>");
  desc_.dirs = kio::ReadBool(is, binary) ? 2 : 1;
  ExpectToken(is, binary, "<RNNMode>");
  desc_.mode = kio::ReadInt(is, binary);
  ExpectToken(is, binary, "<MaxSeqLength>");
  max_seq_length_ = kio::ReadInt(is, binary);
  // InitFromString's checks (nnet-cudnn-component.cc:72-98), before any size is trusted
  if (desc_.mode < 0 || desc_.mode > 3)
    throw std::runtime_error("CuDNNRecurrentComponent: rnn_mode_ = " + std::to_string(desc_.mode) +
                             ", should in [0, 1, 2, 3].");
  if (desc_.D <= 0 || desc_.H <= 0 || desc_.layers <= 0 || max_seq_length_ <= 0)
    throw std::runtime_error("CuDNNRecurrentComponent: bad dimensions in model file");
  ExpectToken(is, binary, "<FilterParams>");
  auto v = kio::ReadFloatVector(is, binary);
  if ((long)v.size() != desc_.params_size())
    throw std::runtime_error("CuDNNRecurrentComponent: FilterParams size mismatch");
  params_.ensure(sizeof(float) * v.size());
  grad_.ensure(sizeof(float) * v.size());
  h2d(params_.f(), v.data(), (long)v.size());
  ExpectToken(is, binary, "</CuDNNRecurrentComponent>");
}

}  // namespace nnet2
}  // namespace kctc
