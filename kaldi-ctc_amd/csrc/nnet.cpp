// nnet.cpp -- the Nnet container of nnet.h (src/nnet2/nnet-nnet.cc).
#include "component_util.h"

namespace kctc {
namespace nnet2 {

Nnet::~Nnet() {
  for (auto *c : components_) delete c;
}

void Nnet::Init(const std::string &config, Rng &rng) {
  std::istringstream is(config);
  std::string line;
  while (std::getline(is, line)) {
    auto hash = line.find('#');
    if (hash != std::string::npos) line = line.substr(0, hash);
    auto parts = split_ws(line);
    if (parts.empty()) continue;
    Component *c = Component::NewComponentOfType(parts[0]);
    if (!c) throw std::invalid_argument("Unknown component type " + parts[0] + " (not on the CTC path)");
    std::string args;
    for (size_t i = 1; i < parts.size(); i++) args += (i > 1 ? " " : "") + parts[i];
    c->InitFromString(args, rng);
    if (!components_.empty() && components_.back()->OutputDim() != c->InputDim()) {
      delete c;
      throw std::invalid_argument("dimension mismatch at component " + parts[0]);
    }
    components_.push_back(c);
  }
  if (components_.empty()) throw std::invalid_argument("empty nnet config");
}

int Nnet::LeftContext() const {  // nnet-nnet.cc:52-64
  int ans = 0;
  for (const Component *c : components_) ans += c->Context().front();
  return -ans;
}
int Nnet::RightContext() const {  // nnet-nnet.cc:66-73
  int ans = 0;
  for (const Component *c : components_) ans += c->Context().back();
  return ans;
}

int Nnet::FirstUpdatableComponent() const {  // nnet-nnet.cc:838-845
  for (int i = 0; i < NumComponents(); i++)
    if (components_[i]->IsUpdatable()) return i;
  return NumComponents();
}

int Nnet::LastUpdatableComponent() const {
  for (int i = NumComponents() - 1; i >= 0; i--)
    if (components_[i]->IsUpdatable()) return i;
  return -1;
}

void Nnet::SetComponent(int c, Component *component) {
  if (c < 0 || c >= NumComponents() || !component) {
    delete component;
    throw std::out_of_range("Nnet::SetComponent: bad index");
  }
  const bool in_ok = c == 0 || components_[c - 1]->OutputDim() == component->InputDim();
  const bool out_ok = c + 1 == NumComponents() || component->OutputDim() == components_[c + 1]->InputDim();
  if (!in_ok || !out_ok || (c > 0 && component->Context() != std::vector<int>{0})) {
    delete component;
    throw std::invalid_argument("Nnet::SetComponent: dimensions or context do not match the neighbours");
  }
  delete components_[c];
  components_[c] = component;
  // packed operands point into the replaced component's reserve
  for (Component *x : components_)
    if (auto *r = dynamic_cast<CuDNNRecurrentComponent *>(x)) r->ClearPackedInput();
}

void Nnet::Insert(int c_to_insert, const std::string &config, Rng &rng) {  // nnet-functions.cc:39-55
  if (c_to_insert < 0 || c_to_insert > NumComponents()) throw std::out_of_range("Nnet::Insert: bad index");
  Nnet src;
  src.Init(config, rng);  // throws on an empty or non-chaining config
  const int ns = src.NumComponents();
  const bool in_ok = c_to_insert == 0 || components_[c_to_insert - 1]->OutputDim() == src.InputDim();
  const bool out_ok = c_to_insert == NumComponents() || src.OutputDim() == components_[c_to_insert]->InputDim();
  if (!in_ok || !out_ok) throw std::invalid_argument("Nnet::Insert: dimensions do not match the neighbours");
  // a component with frame context must stay first (NnetCtcUpdater::SetupChunks)
  for (int c = 0; c < ns; c++)
    if (c_to_insert + c > 0 && src.components_[c]->Context() != std::vector<int>{0})
      throw std::invalid_argument("Nnet::Insert: a component with context other than {0} must come first");
  if (c_to_insert == 0 && !components_.empty() && components_[0]->Context() != std::vector<int>{0})
    throw std::invalid_argument("Nnet::Insert: a component with context other than {0} must come first");
  components_.insert(components_.begin() + c_to_insert, src.components_.begin(), src.components_.end());
  src.components_.clear();  // ownership moved
  if (momentum_ != 0.f) SetMomentum(momentum_);
  for (Component *x : components_)
    if (auto *r = dynamic_cast<CuDNNRecurrentComponent *>(x)) {
      r->ClearPackedInput();
      r->ClearInputBound();
    }
}

void Nnet::ZeroStats() {
  for (auto *c : components_) c->ZeroStats();
}

void Nnet::SetMiniBatch(int N) {
  for (Component *c : components_)
    if (auto *r = dynamic_cast<CuDNNRecurrentComponent *>(c)) r->SetMiniBatch(N);
}

void Nnet::SetMomentum(float m) {
  if (!(m >= 0.f && m < 1.f)) throw std::invalid_argument("momentum must be in [0, 1)");
  momentum_ = m;
  for (auto *c : components_) {
    if (c->IsUpdatable()) static_cast<UpdatableComponent *>(c)->SetMomentum(m);
    if (auto *cg = dynamic_cast<ClipGradientComponent *>(c)) cg->EnableShadow(m != 0.f);
    if (auto *rl = dynamic_cast<RectifiedLinearComponent *>(c)) rl->EnableShadow(m != 0.f);
  }
}

void Nnet::SetDropoutSeed(uint64_t seed) {
  for (int c = 0; c < NumComponents(); c++)
    if (auto *d = dynamic_cast<DropoutComponent *>(components_[c])) d->SetSeed(seed, (uint32_t)c);
}

int Nnet::RemoveDropout() {  // nnet-nnet.cc:507-524
  std::vector<Component *> kept;
  int removed = 0;
  for (Component *c : components_) removed += dynamic_cast<DropoutComponent *>(c) ? 1 : 0;
  if (removed == NumComponents()) throw std::invalid_argument("Nnet::RemoveDropout: nothing but dropout components");
  removed = 0;
  for (Component *c : components_) {
    if (dynamic_cast<DropoutComponent *>(c)) {
      delete c;
      removed++;
    } else {
      kept.push_back(c);
    }
  }
  components_ = kept;
  // Check(): a DropoutComponent has equal input and output dimensions, so the
  // neighbours still chain.  Packed operands and input bounds are set again
  // by the next Propagate for the new neighbours.
  for (Component *x : components_)
    if (auto *r = dynamic_cast<CuDNNRecurrentComponent *>(x)) {
      r->ClearPackedInput();
      r->ClearInputBound();
    }
  return removed;
}

void Nnet::SetDropoutScale(float scale) {  // nnet-nnet.cc:526-538
  for (Component *c : components_)
    if (auto *d = dynamic_cast<DropoutComponent *>(c)) d->SetDropoutScale(scale);
}

void Nnet::SetLearningRate(float lr) {
  for (auto *c : components_)
    if (c->IsUpdatable()) static_cast<UpdatableComponent *>(c)->SetLearningRate(lr);
}

// nnet-nnet.cc:170-183
void Nnet::Write(std::ostream &os, bool binary) const {
  WriteToken(os, binary, "<Nnet>");
  WriteToken(os, binary, "<NumComponents>");
  kio::WriteInt(os, binary, (int32_t)components_.size());
  WriteToken(os, binary, "<Components>");
  for (auto *c : components_) {
    c->Write(os, binary);
    if (!binary) os << "\n";
  }
  WriteToken(os, binary, "</Components>");
  WriteToken(os, binary, "</Nnet>");
}
// nnet-nnet.cc:185-220 (Component::ReadNew: "<Type>" token, then the body)
void Nnet::Read(std::istream &is, bool binary) {
  ExpectToken(is, binary, "<Nnet>");
  ExpectToken(is, binary, "<NumComponents>");
  const int n = kio::ReadInt(is, binary);
  if (n <= 0) throw std::runtime_error("Nnet::Read: <NumComponents> " + std::to_string(n));
  ExpectToken(is, binary, "<Components>");
  for (int i = 0; i < n; i++) components_.push_back(Component::ReadNew(is, binary));
  ExpectToken(is, binary, "</Components>");
  ExpectToken(is, binary, "</Nnet>");
  // Nnet::Read -> Check (nnet-nnet.cc:197-198, 281-289): every component's output feeds the next
  for (int i = 0; i < n; i++) {
    if (components_[i]->InputDim() <= 0 || components_[i]->OutputDim() <= 0)
      throw std::runtime_error("Nnet::Read: component " + std::to_string(i) + " has a non-positive dimension");
    if (i + 1 < n && components_[i]->OutputDim() != components_[i + 1]->InputDim())
      throw std::runtime_error("Nnet::Read: dimension mismatch between components " + std::to_string(i) + " (" +
                               components_[i]->Type() + ", output " + std::to_string(components_[i]->OutputDim()) +
                               ") and " + std::to_string(i + 1) + " (" + components_[i + 1]->Type() + ", input " +
                               std::to_string(components_[i + 1]->InputDim()) + ")");
  }
  SetDropoutSeed(0);  // the file carries no stream identity
}

}  // namespace nnet2
}  // namespace kctc
