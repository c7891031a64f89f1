// component.cpp -- the Component base (Info, NewComponentOfType, ReadNew) and
// UpdatableComponent's parameter arithmetic of nnet.h.
#include "component_util.h"

namespace kctc {
namespace nnet2 {

std::string Component::Info() const {
  std::ostringstream os;
  os << Type() << ", input-dim=" << InputDim() << ", output-dim=" << OutputDim();
  return os.str();
}

void Component::Scale(float) { throw std::invalid_argument(Type() + " has no Scale()"); }
void Component::Add(float, const Component &) { throw std::invalid_argument(Type() + " has no Add()"); }

Component *Component::NewComponentOfType(const std::string &type) {
  if (type == "SpliceComponent") return new SpliceComponent;
  if (type == "CuDNNRecurrentComponent") return new CuDNNRecurrentComponent;
  if (type == "ClipGradientComponent") return new ClipGradientComponent;
  if (type == "AffineComponent") return new AffineComponent;
  if (type == "SoftmaxComponent") return new SoftmaxComponent;
  if (type == "DropoutComponent") return new DropoutComponent;
  if (type == "RectifiedLinearComponent") return new RectifiedLinearComponent;
  if (type == "FixedAffineComponent") return new FixedAffineComponent;
  return nullptr;
}

Component *Component::ReadNew(std::istream &is, bool binary) {
  const std::string t = kio::ReadToken(is, binary);
  if (t.size() < 3 || t.front() != '<' || t.back() != '>') throw std::runtime_error("bad component token " + t);
  Component *c = NewComponentOfType(t.substr(1, t.size() - 2));
  if (!c) throw std::runtime_error("Unknown component type " + t);
  try {
    c->Read(is, binary);
  } catch (...) {
    delete c;
    throw;
  }
  return c;
}

hipStream_t UpdatableComponent::GradStream() const { return grad_stream_ ? grad_stream_ : S(); }

void UpdatableComponent::SetMomentum(float m) {
  if (!(m >= 0.f && m < 1.f)) throw std::invalid_argument("momentum must be in [0, 1)");
  momentum_ = m;
  if (m != 0.f) {  // delta_nnet->SetZero(false): a fresh zero delta
    delta_.ensure(sizeof(float) * NumParameters());
    KCTC_HIP_CHECK(hipMemsetAsync(delta_.p, 0, sizeof(float) * NumParameters(), S()));
  }
}

void UpdatableComponent::UpdateWith(float *params, const float *grad, float clip, const unsigned *skip) {
  if (momentum_ == 0.f)
    clip_sgd_update(S(), params, grad, NumParameters(), learning_rate_, clip, skip);
  else
    momentum_update(S(), params, delta_.f(), grad, NumParameters(), learning_rate_, clip, momentum_, skip);
}

// ---- UpdatableComponent parameter arithmetic (nnet-component.h:295-318) ----
static unsigned long long g_perturb_seed = 20161015ull, g_perturb_calls = 0;
void UpdatableComponent::SetPerturbSeed(unsigned long long seed) {
  g_perturb_seed = seed;
  g_perturb_calls = 0;
}

void UpdatableComponent::CopyUpdatableFrom(const UpdatableComponent &o) {
  learning_rate_ = o.learning_rate_;
  is_gradient_ = o.is_gradient_;
}

void UpdatableComponent::CheckSameKind(const UpdatableComponent &o, const char *what) const {
  if (o.Type() != Type() || o.NumParameters() != NumParameters())
    throw std::invalid_argument(std::string(what) + ": components of different type or size (" + Type() + " vs " +
                                o.Type() + ")");
}

void UpdatableComponent::SetZero(bool treat_as_gradient) {
  if (treat_as_gradient) {
    SetLearningRate(1.0f);
    is_gradient_ = true;
  }
  KCTC_HIP_CHECK(hipMemsetAsync(ParamData(), 0, sizeof(float) * NumParameters(), S()));
}

double UpdatableComponent::DotProduct(const UpdatableComponent &other) const {
  CheckSameKind(other, "DotProduct");
  auto *self = const_cast<UpdatableComponent *>(this);
  auto *o = const_cast<UpdatableComponent *>(&other);
  DevBuf ws;
  ws.ensure(dot_ws_bytes() + sizeof(double));
  double *out = reinterpret_cast<double *>(static_cast<char *>(ws.p) + dot_ws_bytes());
  // the other component's parameters may still be written on its own stream
  KCTC_HIP_CHECK(hipStreamSynchronize(o->GradStream()));
  dot_f64(S(), self->ParamData(), o->ParamData(), NumParameters(), out, ws.p);
  double h = 0;
  KCTC_HIP_CHECK(hipMemcpyAsync(&h, out, sizeof(double), hipMemcpyDeviceToHost, S()));
  KCTC_HIP_CHECK(hipStreamSynchronize(S()));
  return h;
}

void UpdatableComponent::PerturbParams(float stddev) {
  Rng r(g_perturb_seed + 0x51ED27ull * ++g_perturb_calls);
  add_randn(S(), ParamData(), NumParameters(), stddev, r.next());
}

void UpdatableComponent::Scale(float scale) { scale_inplace(S(), ParamData(), NumParameters(), scale); }

void UpdatableComponent::Add(float alpha, const Component &other_in) {
  auto &other = const_cast<UpdatableComponent &>(dynamic_cast<const UpdatableComponent &>(other_in));
  CheckSameKind(other, "Add");
  axpy(S(), ParamData(), other.ParamData(), NumParameters(), alpha);
}

}  // namespace nnet2
}  // namespace kctc
