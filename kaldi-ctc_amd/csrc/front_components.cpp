// front_components.cpp -- the components the recipe's --model-type FT and
// --add-lda put in front of the first RNN (nnet.h): RectifiedLinear and
// FixedAffine.  (The hidden AffineComponent of FT is components.cpp's.)
#include <cmath>

#include "component_util.h"
#include "gemm.h"
#include "nonlinear.h"

namespace kctc {
namespace nnet2 {

// ---------------------------------------------------------------------------
// RectifiedLinearComponent (NonlinearComponent, nnet-component.cc:329-426,
// 798-826)
// ---------------------------------------------------------------------------
RectifiedLinearComponent::~RectifiedLinearComponent() { delete shadow_; }

void RectifiedLinearComponent::SetDim(int dim) {
  dim_ = dim;
  dev_.ensure(sizeof(double) * NumStats());
  KCTC_HIP_CHECK(hipMemsetAsync(dev_.p, 0, sizeof(double) * NumStats(), S()));
  have_value_ = have_deriv_ = false;
  value_sum_.clear();
  deriv_sum_.clear();
  count_ = 0;
}

void RectifiedLinearComponent::InitFromString(std::string args, Rng &) {  // :411-419
  const std::string orig = args;
  int dim = 0;
  const bool ok = ParseFromString("dim", &args, &dim);
  if (!ok || !args.empty() || dim <= 0)
    throw std::invalid_argument("Invalid initializer for layer of type RectifiedLinearComponent: \"" + orig + "\"");
  SetDim(dim);
}

std::string RectifiedLinearComponent::Info() const {
  SyncStats();
  std::ostringstream os;
  os << Component::Info() << ", count=" << count_;
  return os.str();
}

void RectifiedLinearComponent::Propagate(const ChunkInfo &, const ChunkInfo &, const CuMatrixBase &in,
                                         CuMatrixBase *out) const {
  if (in.NumCols() != dim_ || out->NumCols() != dim_ || in.NumRows() != out->NumRows())
    throw std::invalid_argument("RectifiedLinearComponent::Propagate: bad shape");
  ProfScope ps("relu");
  relu_forward(S(), in.Data(), out->Data(), in.NumRows() * (long)dim_);
}

void RectifiedLinearComponent::Backprop(const ChunkInfo &, const ChunkInfo &, const CuMatrixBase &,
                                        const CuMatrixBase &out_value, const CuMatrixBase &out_deriv,
                                        Component *to_update_in, CuMatrixBase *in_deriv) const {
  const long rows = out_value.NumRows();
  if (out_value.NumCols() != dim_ || out_deriv.NumCols() != dim_ || out_deriv.NumRows() != rows ||
      (in_deriv && (in_deriv->NumCols() != dim_ || in_deriv->NumRows() != rows)))
    throw std::invalid_argument("RectifiedLinearComponent::Backprop: bad shape");
  RectifiedLinearComponent *to_update = nullptr;
  if (to_update_in) {
    to_update = dynamic_cast<RectifiedLinearComponent *>(to_update_in);
    if (!to_update || to_update->dim_ != dim_) throw std::invalid_argument("RectifiedLinearComponent: bad to_update");
    // UpdateStats' resizes (:341-354): an absent deriv_sum restarts everything,
    // an absent value_sum restarts itself and the count
    if (!to_update->have_deriv_)
      KCTC_HIP_CHECK(hipMemsetAsync(to_update->dev_.p, 0, sizeof(double) * NumStats(), S()));
    else if (!to_update->have_value_) {
      KCTC_HIP_CHECK(hipMemsetAsync(to_update->Dev(), 0, sizeof(double) * dim_, S()));
      KCTC_HIP_CHECK(hipMemsetAsync(to_update->Dev() + 2L * dim_, 0, sizeof(double), S()));
    }
    to_update->have_value_ = to_update->have_deriv_ = true;
    ws_.ensure(sizeof(float) * relu_stats_ws_floats(rows, dim_));
  }
  if (!in_deriv && !to_update) return;
  ProfScope ps("relu_backprop");
  relu_backprop_stats(S(), out_value.Data(), out_deriv.Data(), in_deriv ? in_deriv->Data() : nullptr, rows, dim_,
                      to_update ? to_update->Dev() : nullptr, to_update ? ws_.f() : nullptr);
}

void RectifiedLinearComponent::SyncStats() const {
  std::vector<double> h((size_t)NumStats());
  KCTC_HIP_CHECK(hipMemcpyAsync(h.data(), dev_.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost, S()));
  KCTC_HIP_CHECK(hipStreamSynchronize(S()));
  value_sum_.clear();
  deriv_sum_.clear();
  if (have_value_) value_sum_.assign(h.begin(), h.begin() + dim_);
  if (have_deriv_) deriv_sum_.assign(h.begin() + dim_, h.begin() + 2L * dim_);
  count_ = h[2L * dim_];
}

Component *RectifiedLinearComponent::Copy() const {  // NonlinearComponent(const NonlinearComponent &) (:405-407)
  auto *c = new RectifiedLinearComponent;
  c->SetDim(dim_);
  c->have_value_ = have_value_;
  c->have_deriv_ = have_deriv_;
  KCTC_HIP_CHECK(hipMemcpyAsync(c->dev_.p, dev_.p, sizeof(double) * NumStats(), hipMemcpyDeviceToDevice, S()));
  return c;
}

void RectifiedLinearComponent::ZeroStats() {  // NonlinearComponent::ZeroStats: the vectors keep their size
  KCTC_HIP_CHECK(hipMemsetAsync(dev_.p, 0, sizeof(double) * NumStats(), S()));
  if (shadow_) shadow_->ZeroStats();
}

void RectifiedLinearComponent::Scale(float scale) {  // :365-369
  stats_axpby(S(), Dev(), nullptr, NumStats(), (double)scale, 0.0);
}

void RectifiedLinearComponent::Add(float alpha, const Component &other_in) {  // :371-382
  const auto &other = dynamic_cast<const RectifiedLinearComponent &>(other_in);
  if (other.dim_ != dim_) throw std::invalid_argument("RectifiedLinearComponent::Add: dimension mismatch");
  // an absent vector is all zero on the device: adding it changes nothing
  have_value_ = have_value_ || other.have_value_;
  have_deriv_ = have_deriv_ || other.have_deriv_;
  stats_axpby(S(), Dev(), other.Dev(), NumStats(), 1.0, (double)alpha);
}

void RectifiedLinearComponent::EnableShadow(bool on) {
  delete shadow_;
  shadow_ = nullptr;
  if (on) {  // delta_nnet = new Nnet(*nnet); delta_nnet->SetZero(false): nc->Scale(0.0)
    shadow_ = static_cast<RectifiedLinearComponent *>(Copy());
    shadow_->Scale(0.f);
  }
}

void RectifiedLinearComponent::FoldShadow(float momentum) {
  if (!shadow_) return;
  have_value_ = have_value_ || shadow_->have_value_;
  have_deriv_ = have_deriv_ || shadow_->have_deriv_;
  stats_fold(S(), Dev(), shadow_->Dev(), NumStats(), (double)momentum);
}

void RectifiedLinearComponent::AllReduceStats(GradExchange &ex, hipStream_t s) {
  ws_.ensure(sizeof(float) * NumStats());
  stats_to_float(s, Dev(), ws_.f(), NumStats());
  ex.AllReduceSum(ws_.f(), NumStats(), s);
  stats_from_float(s, ws_.f(), Dev(), NumStats());
}

// The statistics are written with 17 significant digits in text mode, so a
// text file too gives them back exactly (the reference writes 7; it reads
// either).
void RectifiedLinearComponent::Write(std::ostream &os, bool binary) const {  // :396-409
  SyncStats();
  WriteToken(os, binary, "<RectifiedLinearComponent>");
  WriteToken(os, binary, "<Dim>");
  kio::WriteInt(os, binary, dim_);
  WriteToken(os, binary, "<ValueSum>");
  kio::WriteDoubleVector(os, binary, value_sum_, 17);
  WriteToken(os, binary, "<DerivSum>");
  kio::WriteDoubleVector(os, binary, deriv_sum_, 17);
  WriteToken(os, binary, "<Count>");
  kio::WriteDouble(os, binary, count_, 17);
  WriteToken(os, binary, "</RectifiedLinearComponent>");
}

void RectifiedLinearComponent::Read(std::istream &is, bool binary) {  // :383-394
  ExpectToken(is, binary, "<Dim>");
  const int dim = kio::ReadInt(is, binary);
  if (dim <= 0) throw std::runtime_error("RectifiedLinearComponent: bad <Dim>");
  ExpectToken(is, binary, "<ValueSum>");
  const std::vector<double> v = kio::ReadDoubleVector(is, binary);
  ExpectToken(is, binary, "<DerivSum>");
  const std::vector<double> d = kio::ReadDoubleVector(is, binary);
  ExpectToken(is, binary, "<Count>");
  const double count = kio::ReadDouble(is, binary);
  ExpectToken(is, binary, "</RectifiedLinearComponent>");
  if ((!v.empty() && (int)v.size() != dim) || (!d.empty() && (int)d.size() != dim))
    throw std::runtime_error("RectifiedLinearComponent: statistics of another dimension than <Dim>");
  SetDim(dim);
  std::vector<double> h((size_t)NumStats(), 0.0);
  std::copy(v.begin(), v.end(), h.begin());
  std::copy(d.begin(), d.end(), h.begin() + dim);
  h[2L * dim] = count;
  have_value_ = !v.empty();
  have_deriv_ = !d.empty();
  KCTC_HIP_CHECK(hipMemcpyAsync(dev_.p, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, S()));
  KCTC_HIP_CHECK(hipStreamSynchronize(S()));
}

// ---------------------------------------------------------------------------
// FixedAffineComponent (nnet-component.cc:3274-3363)
// ---------------------------------------------------------------------------
void FixedAffineComponent::Init(const std::vector<float> &linear, const std::vector<float> &bias, int rows,
                                int cols) {
  out_dim_ = rows;
  in_dim_ = cols;
  std::vector<float> h(linear);
  h.insert(h.end(), bias.begin(), bias.end());
  params_.ensure(sizeof(float) * h.size());
  h2d(params_.f(), h.data(), (long)h.size());
}

void FixedAffineComponent::InitFromString(std::string args, Rng &) {  // :3283-3298
  const std::string orig = args;
  std::string filename;
  const bool ok = take("matrix", &args, &filename);
  if (!ok || !args.empty() || filename.empty())
    throw std::invalid_argument("Invalid initializer for layer of type FixedAffineComponent: \"" + orig + "\"");
  std::istringstream is(kio::ReadFile(filename.c_str()));
  const bool binary = kio::InitInput(is);
  int rows = 0, cols = 0;
  const std::vector<float> m = kio::ReadFloatMatrix(is, binary, &rows, &cols);
  // Init (:3274-3280): the last column is the bias
  if (rows <= 0 || cols <= 1)
    throw std::invalid_argument("FixedAffineComponent: " + filename + " holds a " + std::to_string(rows) + " x " +
                                std::to_string(cols) + " matrix (at least one row and two columns are needed)");
  std::vector<float> lin((size_t)rows * (cols - 1)), bias((size_t)rows);
  for (int r = 0; r < rows; r++) {
    std::copy(m.begin() + (size_t)r * cols, m.begin() + (size_t)r * cols + cols - 1, lin.begin() + (size_t)r * (cols - 1));
    bias[r] = m[(size_t)r * cols + cols - 1];
  }
  Init(lin, bias, rows, cols - 1);
}

std::string FixedAffineComponent::Info() const {  // :3301-3316
  const std::vector<float> h = d2h(params_.f(), (long)(in_dim_ + 1) * out_dim_);
  double l2 = 0, b2 = 0;
  const size_t nl = (size_t)in_dim_ * out_dim_;
  for (size_t i = 0; i < nl; i++) l2 += (double)h[i] * h[i];
  for (int i = 0; i < out_dim_; i++) b2 += (double)h[nl + i] * h[nl + i];
  std::ostringstream os;
  os << Component::Info() << ", linear-params-stddev=" << (float)std::sqrt(l2 / (double)nl)
     << ", bias-params-stddev=" << (float)std::sqrt(b2 / out_dim_);
  return os.str();
}

void FixedAffineComponent::Propagate(const ChunkInfo &, const ChunkInfo &, const CuMatrixBase &in,
                                     CuMatrixBase *out) const {  // :3318-3328
  if (in.NumCols() != in_dim_ || out->NumCols() != out_dim_ || in.NumRows() != out->NumRows())
    throw std::invalid_argument("FixedAffineComponent::Propagate: bad shape");
  ProfScope ps("fixed_affine");
  GemmArgs g;
  g.transA = false; g.transB = true;
  g.M = (int)in.NumRows(); g.N = out_dim_; g.K = in_dim_;
  g.A = in.Data(); g.lda = in_dim_;
  g.B = params_.f(); g.ldb = in_dim_;
  g.C = out->Data(); g.ldc = out_dim_;
  g.bias = params_.f() + (long)in_dim_ * out_dim_;
  gemm_f32(S(), g);
}

void FixedAffineComponent::Backprop(const ChunkInfo &, const ChunkInfo &, const CuMatrixBase &, const CuMatrixBase &,
                                    const CuMatrixBase &out_deriv, Component *,
                                    CuMatrixBase *in_deriv) const {  // :3330-3339
  if (!in_deriv) return;
  if (out_deriv.NumCols() != out_dim_ || in_deriv->NumCols() != in_dim_ || in_deriv->NumRows() != out_deriv.NumRows())
    throw std::invalid_argument("FixedAffineComponent::Backprop: bad shape");
  ProfScope ps("fixed_affine");
  GemmArgs g;
  g.M = (int)out_deriv.NumRows(); g.N = in_dim_; g.K = out_dim_;
  g.A = out_deriv.Data(); g.lda = out_dim_;
  g.B = params_.f(); g.ldb = in_dim_;
  g.C = in_deriv->Data(); g.ldc = in_dim_;
  gemm_f32(S(), g);
}

Component *FixedAffineComponent::Copy() const {
  auto *c = new FixedAffineComponent;
  c->in_dim_ = in_dim_;
  c->out_dim_ = out_dim_;
  const size_t P = (size_t)(in_dim_ + 1) * out_dim_;
  c->params_.ensure(sizeof(float) * P);
  KCTC_HIP_CHECK(hipMemcpyAsync(c->params_.p, params_.p, sizeof(float) * P, hipMemcpyDeviceToDevice, S()));
  return c;
}

// Text mode writes the parameters with 9 significant digits: they are not
// trained, so a text model keeps the transform of lda.mat exactly.
void FixedAffineComponent::Write(std::ostream &os, bool binary) const {  // :3349-3356
  const std::vector<float> v = d2h(params_.f(), (long)(in_dim_ + 1) * out_dim_);
  WriteToken(os, binary, "<FixedAffineComponent>");
  WriteToken(os, binary, "<LinearParams>");
  kio::WriteFloatMatrix(os, binary, v.data(), out_dim_, in_dim_, 9);
  WriteToken(os, binary, "<BiasParams>");
  kio::WriteFloatVector(os, binary, v.data() + (size_t)in_dim_ * out_dim_, out_dim_, 9);
  WriteToken(os, binary, "</FixedAffineComponent>");
}

void FixedAffineComponent::Read(std::istream &is, bool binary) {  // :3358-3363
  ExpectToken(is, binary, "<LinearParams>");
  int rows = 0, cols = 0;
  const std::vector<float> lin = kio::ReadFloatMatrix(is, binary, &rows, &cols);
  if (rows <= 0 || cols <= 0) throw std::runtime_error("FixedAffineComponent: empty LinearParams");
  ExpectToken(is, binary, "<BiasParams>");
  const std::vector<float> b = kio::ReadFloatVector(is, binary);
  if ((int)b.size() != rows) throw std::runtime_error("FixedAffineComponent: bias size mismatch");
  ExpectToken(is, binary, "</FixedAffineComponent>");
  Init(lin, b, rows, cols);
}

}  // namespace nnet2
}  // namespace kctc
