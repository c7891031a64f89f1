// components.cpp -- the stateless and small components of nnet.h: Splice,
// ClipGradient, Dropout, Softmax, Affine.
#include "component_util.h"
#include "decodable.h"
#include "dropout.h"
#include "gemm.h"

namespace kctc {
namespace nnet2 {

// ---------------------------------------------------------------------------
// SpliceComponent (nnet-component.cc:2504-2820)
// ---------------------------------------------------------------------------
void SpliceComponent::Init(int input_dim, std::vector<int> context, int const_dim) {  // :2504-2513
  if (context.empty() || input_dim <= 0 || context.front() > 0 || context.back() < 0)
    throw std::invalid_argument("SpliceComponent: context must contain offsets <= 0 and >= 0");
  for (size_t i = 1; i < context.size(); i++)
    if (context[i] <= context[i - 1]) throw std::invalid_argument("SpliceComponent: context must be sorted and unique");
  if (const_dim < 0 || const_dim >= input_dim) throw std::invalid_argument("SpliceComponent: bad const-component-dim");
  input_dim_ = input_dim;
  context_ = std::move(context);
  const_dim_ = const_dim;
}
void SpliceComponent::InitFromString(std::string args, Rng &) {  // :2517-2540
  const std::string orig = args;
  int input_dim = 0, left = 0, right = 0, cdim = 0;
  std::vector<int> context;
  bool in_ok = ParseFromString("input-dim", &args, &input_dim);
  bool ctx_ok = ParseFromString("context", &args, &context);
  bool lr_ok = ParseFromString("left-context", &args, &left) &&
               ParseFromString("right-context", &args, &right);
  ParseFromString("const-component-dim", &args, &cdim);
  if (!(in_ok && (ctx_ok || lr_ok)) || !args.empty() || input_dim <= 0)
    throw std::invalid_argument("Invalid initializer for layer of type SpliceComponent: \"" + orig + "\"");
  if (lr_ok) {
    if (!context.empty()) throw std::invalid_argument("SpliceComponent: context and left/right-context both given");
    for (int i = -left; i <= right; i++) context.push_back(i);
  }
  Init(input_dim, context, cdim);
}
void SpliceComponent::Propagate(const ChunkInfo &in_info, const ChunkInfo &out_info, const CuMatrixBase &in,
                                CuMatrixBase *out) const {
  if (IsIdentityForward()) {
    if (out->Data() != in.Data())
      KCTC_HIP_CHECK(hipMemcpyAsync(out->Data(), in.Data(), sizeof(float) * in.NumRows() * in.NumCols(),
                                    hipMemcpyDeviceToDevice, S()));
    return;
  }
  const long rows = out->NumRows();
  if (rows <= 0 || in.NumRows() % rows) throw std::invalid_argument("SpliceComponent: input rows are not chunks of the output rows");
  const int ns = (int)(in.NumRows() / rows);
  // input row of output frame j for context offset 0: j * ns + (out offset - in offset)
  const int first = out_info.first_offset - in_info.first_offset;
  if (first + context_.front() < 0 || first + context_.back() >= ns)
    throw std::invalid_argument("SpliceComponent: context outside the input chunk");
  splice_rows(S(), in.Data(), input_dim_, ns, rows, context_.data(), (int)context_.size(), first, const_dim_,
              out->Data());
}
void SpliceComponent::Backprop(const ChunkInfo &in_info, const ChunkInfo &out_info, const CuMatrixBase &,
                               const CuMatrixBase &, const CuMatrixBase &out_deriv, Component *,
                               CuMatrixBase *in_deriv) const {  // :2691-2760
  if (!in_deriv) return;
  if (IsIdentityForward()) {
    if (in_deriv->Data() != out_deriv.Data())
      KCTC_HIP_CHECK(hipMemcpyAsync(in_deriv->Data(), out_deriv.Data(),
                                    sizeof(float) * out_deriv.NumRows() * out_deriv.NumCols(),
                                    hipMemcpyDeviceToDevice, S()));
    return;
  }
  const long rows = out_deriv.NumRows();
  const int ns = (int)(in_deriv->NumRows() / rows);
  splice_rows_backward(S(), out_deriv.Data(), input_dim_, ns, rows, context_.data(), (int)context_.size(),
                       out_info.first_offset - in_info.first_offset, const_dim_, in_deriv->Data());
}
Component *SpliceComponent::Copy() const {
  auto *c = new SpliceComponent;
  c->input_dim_ = input_dim_;
  c->const_dim_ = const_dim_;
  c->context_ = context_;
  return c;
}
void SpliceComponent::Write(std::ostream &os, bool binary) const {  // :2822-2833
  WriteToken(os, binary, "<SpliceComponent>");
  WriteToken(os, binary, "<InputDim>");
  kio::WriteInt(os, binary, input_dim_);
  WriteToken(os, binary, "<Context>");
  kio::WriteIntVector(os, binary, std::vector<int32_t>(context_.begin(), context_.end()));
  WriteToken(os, binary, "<ConstComponentDim>");
  kio::WriteInt(os, binary, const_dim_);
  WriteToken(os, binary, "</SpliceComponent>");
}
// SpliceComponent::Read (nnet-component.cc:2797-2820), incl. the old
// <LeftContext>/<RightContext> form
void SpliceComponent::Read(std::istream &is, bool binary) {
  ExpectToken(is, binary, "<InputDim>");
  const int input_dim = kio::ReadInt(is, binary);
  const std::string t = kio::ReadToken(is, binary);
  std::vector<int> context;
  if (t == "<LeftContext>") {
    const int l = kio::ReadInt(is, binary);
    ExpectToken(is, binary, "<RightContext>");
    const int r = kio::ReadInt(is, binary);
    for (int i = -l; i <= r; i++) context.push_back(i);
  } else if (t == "<Context>") {
    for (int32_t c : kio::ReadIntVector(is, binary)) context.push_back(c);
  } else {
    throw std::runtime_error("SpliceComponent: unknown token " + t);
  }
  ExpectToken(is, binary, "<ConstComponentDim>");
  const int cdim = kio::ReadInt(is, binary);
  ExpectToken(is, binary, "</SpliceComponent>");
  if (input_dim <= 0) throw std::runtime_error("SpliceComponent: bad <InputDim>");
  Init(input_dim, context, cdim);
}

// ---------------------------------------------------------------------------
// ClipGradientComponent (nnet-cudnn-component.cc:775-1075)
// ---------------------------------------------------------------------------
ClipGradientComponent::ClipGradientComponent() {
  KCTC_HIP_CHECK(hipMalloc(&dev_, sizeof(ClipState)));
  KCTC_HIP_CHECK(hipMemset(dev_, 0, sizeof(ClipState)));
}
ClipGradientComponent::~ClipGradientComponent() {
  delete shadow_;
  if (dev_) (void)hipFree(dev_);
}

// delta_nnet = new Nnet(*nnet): the copy starts with this component's
// configuration and counters (ctc-nnet-train.cc:194-202)
void ClipGradientComponent::EnableShadow(bool on) {
  delete shadow_;
  shadow_ = nullptr;
  if (on) shadow_ = static_cast<ClipGradientComponent *>(Copy());
}

void ClipGradientComponent::InitFromString(std::string args, Rng &) {
  const std::string orig = args;
  bool ok = ParseFromString("dim", &args, &dim_);
  clipping_threshold_ = 15.0f;
  norm_based_clipping_ = false;
  self_repair_clipped_proportion_threshold_ = 0.01f;
  self_repair_target_ = 0.0f;
  self_repair_scale_ = 1.0f;
  ParseFromString("clipping-threshold", &args, &clipping_threshold_);
  ParseFromString("norm-based-clipping", &args, &norm_based_clipping_);
  ParseFromString("self-repair-clipped-proportion-threshold", &args,
                  &self_repair_clipped_proportion_threshold_);
  ParseFromString("self-repair-target", &args, &self_repair_target_);
  ParseFromString("self-repair-scale", &args, &self_repair_scale_);
  if (!ok || !args.empty() || clipping_threshold_ < 0 || dim_ <= 0 ||
      self_repair_clipped_proportion_threshold_ < 0 || self_repair_target_ < 0 ||
      self_repair_scale_ < 0)
    throw std::invalid_argument("Invalid initializer for layer of type ClipGradientComponent: \"" +
                                orig + "\"");
  ZeroStats();
}

std::string ClipGradientComponent::Info() const {
  SyncStats();
  std::ostringstream os;
  os << Type() << ", dim=" << dim_ << ", norm-based-clipping=" << (norm_based_clipping_ ? "true" : "false")
     << ", clipping-threshold=" << clipping_threshold_
     << ", clipped-proportion=" << (count_ > 0 ? num_clipped_ / count_ : 0.0);
  if (self_repair_scale_ != 0.0f)
    os << ", self-repair-clipped-proportion-threshold=" << self_repair_clipped_proportion_threshold_
       << ", self-repair-target=" << self_repair_target_ << ", self-repair-scale=" << self_repair_scale_;
  return os.str();
}

void ClipGradientComponent::Propagate(const ChunkInfo &, const ChunkInfo &, const CuMatrixBase &in,
                                      CuMatrixBase *out) const {
  if (out->Data() != in.Data())
    KCTC_HIP_CHECK(hipMemcpyAsync(out->Data(), in.Data(), sizeof(float) * in.NumRows() * in.NumCols(),
                                  hipMemcpyDeviceToDevice, S()));
}

void ClipGradientComponent::Backprop(const ChunkInfo &, const ChunkInfo &, const CuMatrixBase &in_value,
                                     const CuMatrixBase &, const CuMatrixBase &out_deriv,
                                     Component *to_update_in, CuMatrixBase *in_deriv) const {
  if (!in_deriv) return;
  if (in_deriv->Data() != out_deriv.Data())
    KCTC_HIP_CHECK(hipMemcpyAsync(in_deriv->Data(), out_deriv.Data(),
                                  sizeof(float) * out_deriv.NumRows() * out_deriv.NumCols(),
                                  hipMemcpyDeviceToDevice, S()));
  auto *to_update = dynamic_cast<ClipGradientComponent *>(to_update_in);
  if (!(clipping_threshold_ > 0)) return;
  const long rows = in_deriv->NumRows();
  // RepairGradients' host-side gate, in the reference's short-circuit order
  // (:988-991): the RandUniform() draw is consumed only when the preceding
  // conditions pass.  count_ includes this minibatch when norm-based.
  bool try_repair = false;
  if (to_update) {
    to_update->num_backpropped_ += 1;
    const double count_after = count_ + ((norm_based_clipping_ && to_update == this) ? rows : 0);
    if (!(self_repair_clipped_proportion_threshold_ >= 1.0f || self_repair_scale_ == 0.0f ||
          count_after == 0)) {
      if (!rng_) throw std::logic_error("ClipGradientComponent: no random stream for self-repair");
      try_repair = !(rng_->RandUniform() > 0.5f);  // RandUniform() > repair_probability
    }
    if (norm_based_clipping_) to_update->count_ += rows;
  }
  ProfScope ps("clip_gradient");
  scratch_.ensure(clipgrad_scratch_bytes(rows));
  clipgrad_backprop(S(), in_deriv->Data(), in_value.Data(), rows, dim_, clipping_threshold_,
                    norm_based_clipping_, try_repair, self_repair_clipped_proportion_threshold_,
                    self_repair_target_, self_repair_scale_, to_update ? to_update->dev_ : nullptr,
                    scratch_.p, dev_);
}

Component *ClipGradientComponent::Copy() const {
  auto *c = new ClipGradientComponent;
  c->dim_ = dim_;
  c->clipping_threshold_ = clipping_threshold_;
  c->norm_based_clipping_ = norm_based_clipping_;
  c->self_repair_clipped_proportion_threshold_ = self_repair_clipped_proportion_threshold_;
  c->self_repair_target_ = self_repair_target_;
  c->self_repair_scale_ = self_repair_scale_;
  SyncStats();
  c->num_clipped_ = num_clipped_;
  c->count_ = count_;
  c->num_self_repaired_ = num_self_repaired_;
  c->num_backpropped_ = num_backpropped_;
  KCTC_HIP_CHECK(hipMemcpyAsync(c->dev_, dev_, sizeof(ClipState), hipMemcpyDeviceToDevice, S()));
  return c;
}

// the device counters are the truth during training; scaled on the host and
// written back (both are off the per-step path)
void ClipGradientComponent::Scale(float scale) {  // :1064-1067
  SyncStats();
  count_ *= scale;
  num_clipped_ *= scale;
  ClipState h{};
  h.num_clipped = num_clipped_;
  h.count = count_;
  h.num_self_repaired = num_self_repaired_;
  KCTC_HIP_CHECK(hipMemcpyAsync(dev_, &h, sizeof(h), hipMemcpyHostToDevice, S()));
  KCTC_HIP_CHECK(hipStreamSynchronize(S()));
}

void ClipGradientComponent::Add(float alpha, const Component &other_in) {  // :1069-1073
  const auto &other = dynamic_cast<const ClipGradientComponent &>(other_in);
  SyncStats();
  other.SyncStats();
  count_ += alpha * other.count_;
  num_clipped_ += alpha * other.num_clipped_;
  ClipState h{};
  h.num_clipped = num_clipped_;
  h.count = count_;
  h.num_self_repaired = num_self_repaired_;
  KCTC_HIP_CHECK(hipMemcpyAsync(dev_, &h, sizeof(h), hipMemcpyHostToDevice, S()));
  KCTC_HIP_CHECK(hipStreamSynchronize(S()));
}

void ClipGradientComponent::SyncStats() const {
  ClipState h;
  KCTC_HIP_CHECK(hipMemcpyAsync(&h, dev_, sizeof(h), hipMemcpyDeviceToHost, S()));
  KCTC_HIP_CHECK(hipStreamSynchronize(S()));
  num_clipped_ = h.num_clipped;
  count_ = h.count;
  num_self_repaired_ = h.num_self_repaired;
}

void ClipGradientComponent::ZeroStats() {
  KCTC_HIP_CHECK(hipMemsetAsync(dev_, 0, sizeof(ClipState), S()));
  num_clipped_ = count_ = num_self_repaired_ = num_backpropped_ = 0;
}

// nnet-cudnn-component.cc:814-837
void ClipGradientComponent::Write(std::ostream &os, bool binary) const {
  SyncStats();
  WriteToken(os, binary, "<ClipGradientComponent>");
  WriteToken(os, binary, "<Dim>");
  kio::WriteInt(os, binary, dim_);
  WriteToken(os, binary, "<ClippingThreshold>");
  kio::WriteFloat(os, binary, clipping_threshold_);
  WriteToken(os, binary, "<NormBasedClipping>");
  kio::WriteBool(os, binary, norm_based_clipping_);
  WriteToken(os, binary, "<SelfRepairClippedProportionThreshold>");
  kio::WriteFloat(os, binary, self_repair_clipped_proportion_threshold_);
  WriteToken(os, binary, "<SelfRepairTarget>");
  kio::WriteFloat(os, binary, self_repair_target_);
  WriteToken(os, binary, "<SelfRepairScale>");
  kio::WriteFloat(os, binary, self_repair_scale_);
  WriteToken(os, binary, "<NumElementsClipped>");
  kio::WriteInt(os, binary, as_i32(num_clipped_));
  WriteToken(os, binary, "<NumElementsProcessed>");
  kio::WriteInt(os, binary, as_i32(count_));
  WriteToken(os, binary, "<NumSelfRepaired>");
  kio::WriteInt(os, binary, as_i32(num_self_repaired_));
  WriteToken(os, binary, "<NumBackpropped>");
  kio::WriteInt(os, binary, as_i32(num_backpropped_));
  WriteToken(os, binary, "</ClipGradientComponent>");
}// nnet-cudnn-component.cc:775-812 (older files without the self-repair fields)
void ClipGradientComponent::Read(std::istream &is, bool binary) {
  ExpectToken(is, binary, "<Dim>");
  dim_ = kio::ReadInt(is, binary);
  ExpectToken(is, binary, "<ClippingThreshold>");
  clipping_threshold_ = kio::ReadFloat(is, binary);
  ExpectToken(is, binary, "<NormBasedClipping>");
  norm_based_clipping_ = kio::ReadBool(is, binary);
  std::string t = kio::ReadToken(is, binary);
  if (t == "<SelfRepairClippedProportionThreshold>") {
    self_repair_clipped_proportion_threshold_ = kio::ReadFloat(is, binary);
    ExpectToken(is, binary, "<SelfRepairTarget>");
    self_repair_target_ = kio::ReadFloat(is, binary);
    ExpectToken(is, binary, "<SelfRepairScale>");
    self_repair_scale_ = kio::ReadFloat(is, binary);
    ExpectToken(is, binary, "<NumElementsClipped>");
  } else {
    self_repair_clipped_proportion_threshold_ = 1.0f;
    self_repair_target_ = 0.0f;
    self_repair_scale_ = 0.0f;
    if (t != "<NumElementsClipped>") throw std::runtime_error("ClipGradientComponent: bad token " + t);
  }
  num_clipped_ = kio::ReadInt(is, binary);
  ExpectToken(is, binary, "<NumElementsProcessed>");
  count_ = kio::ReadInt(is, binary);
  t = kio::ReadToken(is, binary);
  if (t == "<NumSelfRepaired>") {
    num_self_repaired_ = kio::ReadInt(is, binary);
    ExpectToken(is, binary, "<NumBackpropped>");
    num_backpropped_ = kio::ReadInt(is, binary);
    ExpectToken(is, binary, "</ClipGradientComponent>");
  } else {
    num_self_repaired_ = num_backpropped_ = 0;
    if (t != "</ClipGradientComponent>") throw std::runtime_error("ClipGradientComponent: bad token " + t);
  }
  ClipState h{};
  h.num_clipped = num_clipped_;
  h.count = count_;
  h.num_self_repaired = num_self_repaired_;
  KCTC_HIP_CHECK(hipMemcpy(dev_, &h, sizeof(h), hipMemcpyHostToDevice));
}
// ---------------------------------------------------------------------------
// DropoutComponent (nnet-component.cc:3508-3611)
// ---------------------------------------------------------------------------
// the reference asserts these in Propagate (:3570-3571)
void DropoutComponent::Check(float proportion, float scale) {
  if (!(proportion >= 0.f && proportion < 1.f))
    throw std::invalid_argument("DropoutComponent: dropout-proportion must be in [0, 1)");
  if (!(scale >= 0.f && scale <= 1.f)) throw std::invalid_argument("DropoutComponent: dropout-scale must be in [0, 1]");
}
void DropoutComponent::InitFromString(std::string args, Rng &) {  // :3516-3528
  const std::string orig = args;
  int dim = 0;
  float proportion = 0.5f, scale = 0.0f;
  const bool ok = ParseFromString("dim", &args, &dim);
  ParseFromString("dropout-proportion", &args, &proportion);
  ParseFromString("dropout-scale", &args, &scale);
  if (!ok || !args.empty() || dim <= 0)
    throw std::invalid_argument("Invalid initializer for layer of type DropoutComponent: \"" + orig + "\"");
  Check(proportion, scale);
  dim_ = dim;
  dropout_proportion_ = proportion;
  dropout_scale_ = scale;
  draw_ = 0;
}
void DropoutComponent::SetDropoutScale(float scale) {
  Check(dropout_proportion_, scale);
  dropout_scale_ = scale;
}
std::string DropoutComponent::Info() const {
  std::ostringstream os;
  os << Type() << ", dim=" << dim_ << ", dropout-proportion=" << dropout_proportion_
     << ", dropout-scale=" << dropout_scale_;
  return os.str();
}
void DropoutComponent::Propagate(const ChunkInfo &, const ChunkInfo &, const CuMatrixBase &in,
                                 CuMatrixBase *out) const {
  if (in.NumCols() != dim_ || out->NumCols() != dim_ || in.NumRows() != out->NumRows())
    throw std::invalid_argument("DropoutComponent::Propagate: bad shape");
  ProfScope ps("dropout");
  DropoutMask m;
  m.seed = seed_; m.stream = stream_; m.draw = draw_++;
  m.proportion = dropout_proportion_; m.scale = dropout_scale_;
  dropout_forward(S(), in.Data(), out->Data(), in.NumRows() * (long)dim_, m);
}
void DropoutComponent::Backprop(const ChunkInfo &, const ChunkInfo &, const CuMatrixBase &, const CuMatrixBase &,
                                const CuMatrixBase &out_deriv, Component *, CuMatrixBase *in_deriv) const {
  if (!in_deriv) return;
  if (out_deriv.NumCols() != dim_ || in_deriv->NumCols() != dim_ || in_deriv->NumRows() != out_deriv.NumRows())
    throw std::invalid_argument("DropoutComponent::Backprop: bad shape");
  if (draw_ == 0) throw std::logic_error("DropoutComponent::Backprop before any Propagate (no mask was drawn)");
  ProfScope ps("dropout");
  DropoutMask m;
  m.seed = seed_; m.stream = stream_; m.draw = draw_ - 1;  // the last Propagate's
  m.proportion = dropout_proportion_; m.scale = dropout_scale_;
  dropout_backward(S(), out_deriv.Data(), in_deriv->Data(), out_deriv.NumRows() * (long)dim_, m);
}
Component *DropoutComponent::Copy() const {
  auto *c = new DropoutComponent;
  c->dim_ = dim_;
  c->dropout_proportion_ = dropout_proportion_;
  c->dropout_scale_ = dropout_scale_;
  c->seed_ = seed_;
  c->stream_ = stream_;
  c->draw_ = draw_;
  return c;
}
void DropoutComponent::Write(std::ostream &os, bool binary) const {  // :3540-3549
  WriteToken(os, binary, "<DropoutComponent>");
  WriteToken(os, binary, "<Dim>");
  kio::WriteInt(os, binary, dim_);
  WriteToken(os, binary, "<DropoutScale>");
  kio::WriteFloat(os, binary, dropout_scale_);
  WriteToken(os, binary, "<DropoutProportion>");
  kio::WriteFloat(os, binary, dropout_proportion_);
  WriteToken(os, binary, "</DropoutComponent>");
}
void DropoutComponent::Read(std::istream &is, bool binary) {  // :3530-3538
  ExpectToken(is, binary, "<Dim>");
  dim_ = kio::ReadInt(is, binary);
  if (dim_ <= 0) throw std::runtime_error("DropoutComponent: bad <Dim>");
  ExpectToken(is, binary, "<DropoutScale>");
  dropout_scale_ = kio::ReadFloat(is, binary);
  ExpectToken(is, binary, "<DropoutProportion>");
  dropout_proportion_ = kio::ReadFloat(is, binary);
  ExpectToken(is, binary, "</DropoutComponent>");
  Check(dropout_proportion_, dropout_scale_);
  seed_ = 0;
  stream_ = 0;
  draw_ = 0;
}
// ---------------------------------------------------------------------------
// SoftmaxComponent (NonlinearComponent I/O, nnet-component.cc:383-426)
// ---------------------------------------------------------------------------
void SoftmaxComponent::InitFromString(std::string args, Rng &) {
  const std::string orig = args;
  const bool ok = ParseFromString("dim", &args, &dim_);
  if (!ok || !args.empty() || dim_ <= 0)
    throw std::invalid_argument("Invalid initializer for layer of type SoftmaxComponent: \"" + orig + "\"");
  value_sum_.clear();
  deriv_sum_.clear();
  count_ = 0;
}
void SoftmaxComponent::Propagate(const ChunkInfo &, const ChunkInfo &, const CuMatrixBase &in,
                                 CuMatrixBase *out) const {
  ProfScope ps("softmax");
  softmax_rows(S(), in.Data(), in.NumRows(), dim_, out->Data());  // ApplySoftMaxPerRow + ApplyFloor(1e-20)
}
void SoftmaxComponent::Backprop(const ChunkInfo &, const ChunkInfo &, const CuMatrixBase &,
                                const CuMatrixBase &out_value, const CuMatrixBase &out_deriv, Component *to_update_in,
                                CuMatrixBase *in_deriv) const {
  const long rows = out_deriv.NumRows();
  if (in_deriv) diff_softmax_rows(S(), out_value.Data(), out_deriv.Data(), rows, dim_, in_deriv->Data());
  if (to_update_in) {  // NonlinearComponent::UpdateStats(out_value) (:337-363): value_sum_ += column sums, count_ += rows
    auto *to_update = dynamic_cast<SoftmaxComponent *>(to_update_in);
    if (!to_update) throw std::invalid_argument("SoftmaxComponent: bad to_update");
    ws_.ensure(sizeof(float) * ((size_t)dim_ + sum_rows_ws_floats(rows, dim_)));
    sum_rows(S(), out_value.Data(), rows, dim_, 1.f, 0.f, ws_.f(), ws_.f() + dim_);
    auto v = d2h(ws_.f(), dim_);
    if (to_update->value_sum_.empty()) to_update->value_sum_.assign(dim_, 0.0);
    for (int j = 0; j < dim_; j++) to_update->value_sum_[j] += v[j];
    to_update->count_ += (double)rows;
  }
}
Component *SoftmaxComponent::Copy() const {
  auto *c = new SoftmaxComponent;
  c->dim_ = dim_;
  c->value_sum_ = value_sum_;
  c->deriv_sum_ = deriv_sum_;
  c->count_ = count_;
  return c;
}
void SoftmaxComponent::Scale(float scale) {  // NonlinearComponent::Scale (nnet-component.cc:365-369)
  for (auto &v : value_sum_) v *= scale;
  for (auto &v : deriv_sum_) v *= scale;
  count_ *= scale;
}
void SoftmaxComponent::Add(float alpha, const Component &other_in) {  // NonlinearComponent::Add (:371-382)
  const auto &other = dynamic_cast<const SoftmaxComponent &>(other_in);
  if (value_sum_.empty() && !other.value_sum_.empty()) value_sum_.assign(other.value_sum_.size(), 0.0);
  if (deriv_sum_.empty() && !other.deriv_sum_.empty()) deriv_sum_.assign(other.deriv_sum_.size(), 0.0);
  for (size_t j = 0; j < other.value_sum_.size() && j < value_sum_.size(); j++) value_sum_[j] += alpha * other.value_sum_[j];
  for (size_t j = 0; j < other.deriv_sum_.size() && j < deriv_sum_.size(); j++) deriv_sum_[j] += alpha * other.deriv_sum_[j];
  count_ += alpha * other.count_;
}
void SoftmaxComponent::Write(std::ostream &os, bool binary) const {
  WriteToken(os, binary, "<SoftmaxComponent>");
  WriteToken(os, binary, "<Dim>");
  kio::WriteInt(os, binary, dim_);
  WriteToken(os, binary, "<ValueSum>");
  kio::WriteDoubleVector(os, binary, value_sum_);
  WriteToken(os, binary, "<DerivSum>");
  kio::WriteDoubleVector(os, binary, deriv_sum_);
  WriteToken(os, binary, "<Count>");
  kio::WriteDouble(os, binary, count_);
  WriteToken(os, binary, "</SoftmaxComponent>");
}
void SoftmaxComponent::Read(std::istream &is, bool binary) {
  // ExpectOneOrTwoTokens(<SoftmaxComponent>, <Dim>): the type token was consumed by Nnet::Read
  ExpectToken(is, binary, "<Dim>");
  dim_ = kio::ReadInt(is, binary);
  if (dim_ <= 0) throw std::runtime_error("SoftmaxComponent: bad <Dim>");
  ExpectToken(is, binary, "<ValueSum>");
  value_sum_ = kio::ReadDoubleVector(is, binary);
  ExpectToken(is, binary, "<DerivSum>");
  deriv_sum_ = kio::ReadDoubleVector(is, binary);
  ExpectToken(is, binary, "<Count>");
  count_ = kio::ReadDouble(is, binary);
  ExpectToken(is, binary, "</SoftmaxComponent>");
}
// ---------------------------------------------------------------------------
// AffineComponent (nnet-component.cc:1125-1274)
// ---------------------------------------------------------------------------
void AffineComponent::InitFromString(std::string args, Rng &rng) {
  const std::string orig = args;
  bool ok = true;
  ParseFromString("learning-rate", &args, &learning_rate_);
  ok = ok && ParseFromString("input-dim", &args, &in_dim_);
  ok = ok && ParseFromString("output-dim", &args, &out_dim_);
  if (!ok || in_dim_ <= 0 || out_dim_ <= 0) throw std::invalid_argument("Bad initializer " + orig);
  float param_stddev = 1.0f / std::sqrt((float)in_dim_), bias_stddev = 1.0f;
  ParseFromString("param-stddev", &args, &param_stddev);
  ParseFromString("bias-stddev", &args, &bias_stddev);
  if (!args.empty()) throw std::invalid_argument("Could not process these elements in initializer: " + args);
  std::vector<float> h((size_t)NumParameters());
  for (long i = 0; i < (long)in_dim_ * out_dim_; i++) h[i] = (float)(rng.gauss() * param_stddev);
  for (int i = 0; i < out_dim_; i++) h[(long)in_dim_ * out_dim_ + i] = (float)(rng.gauss() * bias_stddev);
  params_.ensure(sizeof(float) * h.size());
  grad_.ensure(sizeof(float) * h.size());
  h2d(params_.f(), h.data(), (long)h.size());
}

std::string AffineComponent::Info() const {
  std::ostringstream os;
  os << Type() << ", input-dim=" << in_dim_ << ", output-dim=" << out_dim_
     << ", learning-rate=" << learning_rate_;
  return os.str();
}

void AffineComponent::Propagate(const ChunkInfo &, const ChunkInfo &, const CuMatrixBase &in,
                                CuMatrixBase *out) const {
  // out = 1 b^T + in W^T (CopyRowsFromVec + AddMatMat, :1184-1196), fused bias
  ProfScope ps("affine");
  GemmArgs g;
  g.transA = false; g.transB = true;
  g.M = (int)in.NumRows(); g.N = out_dim_; g.K = in_dim_;
  g.A = in.Data(); g.lda = in_dim_;
  g.B = params_.f(); g.ldb = in_dim_;
  g.C = out->Data(); g.ldc = out_dim_;
  g.bias = params_.f() + (long)in_dim_ * out_dim_;
  gemm_f32(S(), g);
}

void AffineComponent::Backprop(const ChunkInfo &, const ChunkInfo &, const CuMatrixBase &in_value,
                               const CuMatrixBase &, const CuMatrixBase &out_deriv,
                               Component *to_update_in, CuMatrixBase *in_deriv) const {
  ProfScope ps("affine");
  const long rows = out_deriv.NumRows();
  if (in_deriv) {  // in_deriv = out_deriv W
    GemmArgs g;
    g.M = (int)rows; g.N = in_dim_; g.K = out_dim_;
    g.A = out_deriv.Data(); g.lda = out_dim_;
    g.B = params_.f(); g.ldb = in_dim_;
    g.C = in_deriv->Data(); g.ldc = in_dim_;
    gemm_f32(S(), g);
  }
  if (to_update_in) {
    auto *to_update = dynamic_cast<AffineComponent *>(to_update_in);
    if (!to_update) throw std::invalid_argument("AffineComponent: bad to_update");
    // UpdateSimple (:1190-1195): grad_W = out_deriv^T in_value, grad_b = row sum
    GemmArgs g;
    g.transA = true;
    g.M = out_dim_; g.N = in_dim_; g.K = (int)rows;
    g.A = out_deriv.Data(); g.lda = out_dim_;
    g.B = in_value.Data(); g.ldb = in_dim_;
    g.C = to_update->grad_.f(); g.ldc = in_dim_;
    g.split_k = gemm_pick_split(g.M, g.N, g.K, 1);
    const size_t wsf = (size_t)g.split_k * g.M * g.N + sum_rows_ws_floats(rows, out_dim_);
    ws_.ensure(sizeof(float) * wsf);
    g.ws = ws_.f();
    gemm_f32(S(), g);
    sum_rows(S(), out_deriv.Data(), rows, out_dim_, 1.f, 0.f,
             to_update->grad_.f() + (long)in_dim_ * out_dim_, ws_.f() + (size_t)g.split_k * g.M * g.N);
  }
}

Component *AffineComponent::Copy() const {  // AffineComponent(const AffineComponent &) (:1046-1050)
  auto *c = new AffineComponent;
  c->CopyUpdatableFrom(*this);
  c->in_dim_ = in_dim_;
  c->out_dim_ = out_dim_;
  const long P = NumParameters();
  c->params_.ensure(sizeof(float) * P);
  c->grad_.ensure(sizeof(float) * P);
  KCTC_HIP_CHECK(hipMemcpyAsync(c->params_.p, params_.p, sizeof(float) * P, hipMemcpyDeviceToDevice, S()));
  return c;
}

void AffineComponent::ApplyUpdate(const unsigned *skip) {
  UpdateWith(params_.f(), grad_.f(), 0.f, skip);
}
void AffineComponent::Vectorize(float *host) const {
  auto v = d2h(params_.f(), NumParameters());
  std::copy(v.begin(), v.end(), host);
}
void AffineComponent::UnVectorize(const float *host) { h2d(params_.f(), host, NumParameters()); }

// nnet-component.cc:1260-1274
void AffineComponent::Write(std::ostream &os, bool binary) const {
  auto v = d2h(params_.f(), NumParameters());
  WriteToken(os, binary, "<AffineComponent>");
  WriteToken(os, binary, "<LearningRate>");
  kio::WriteFloat(os, binary, learning_rate_);
  WriteToken(os, binary, "<LinearParams>");
  kio::WriteFloatMatrix(os, binary, v.data(), out_dim_, in_dim_);
  WriteToken(os, binary, "<BiasParams>");
  kio::WriteFloatVector(os, binary, v.data() + (long)in_dim_ * out_dim_, out_dim_);
  WriteToken(os, binary, "<IsGradient>");
  kio::WriteBool(os, binary, is_gradient_);
  WriteToken(os, binary, "</AffineComponent>");
}// nnet-component.cc:1228-1258 (incl. the <AvgInput> back-compatibility fields)
void AffineComponent::Read(std::istream &is, bool binary) {
  ExpectToken(is, binary, "<LearningRate>");
  learning_rate_ = kio::ReadFloat(is, binary);
  ExpectToken(is, binary, "<LinearParams>");
  int rows = 0, cols = 0;
  auto lin = kio::ReadFloatMatrix(is, binary, &rows, &cols);
  if (rows == 0 || cols == 0) throw std::runtime_error("AffineComponent: empty LinearParams");
  out_dim_ = rows;
  in_dim_ = cols;
  ExpectToken(is, binary, "<BiasParams>");
  auto b = kio::ReadFloatVector(is, binary);
  if ((int)b.size() != out_dim_) throw std::runtime_error("AffineComponent: bias size mismatch");
  std::string t = kio::ReadToken(is, binary);
  if (t == "<AvgInput>") {  // discarded
    kio::ReadFloatVector(is, binary);
    ExpectToken(is, binary, "<AvgInputCount>");
    kio::ReadFloat(is, binary);
    t = kio::ReadToken(is, binary);
  }
  is_gradient_ = false;
  if (t == "<IsGradient>") {
    is_gradient_ = kio::ReadBool(is, binary);
    t = kio::ReadToken(is, binary);
  }
  if (t != "</AffineComponent>") throw std::runtime_error("AffineComponent: bad token " + t);
  lin.insert(lin.end(), b.begin(), b.end());
  params_.ensure(sizeof(float) * lin.size());
  grad_.ensure(sizeof(float) * lin.size());
  h2d(params_.f(), lin.data(), (long)lin.size());
}

}  // namespace nnet2
}  // namespace kctc
