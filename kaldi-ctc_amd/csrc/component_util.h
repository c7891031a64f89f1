// component_util.h -- what the component, network and updater sources share:
// the compute stream, profiling scopes, host <-> device copies and the
// config-line parser.
#pragma once
#include <sstream>

#include "common.h"
#include "elementwise.h"
#include "kaldi_io.h"
#include "nnet.h"

namespace kctc {
namespace nnet2 {

struct ProfScope {
  explicit ProfScope(const char *f, hipStream_t s = nullptr) { CuDevice::Instantiate().Begin(f, s); }
  ~ProfScope() { CuDevice::Instantiate().End(); }
};

inline hipStream_t S() { return CuDevice::Instantiate().stream; }

// ---- config parsing: ParseFromString (src/nnet2/nnet-component.cc:160-260) ----
inline std::vector<std::string> split_ws(const std::string &s) {
  std::vector<std::string> out;
  std::istringstream is(s);
  std::string t;
  while (is >> t) out.push_back(t);
  return out;
}

inline bool take(const std::string &name, std::string *args, std::string *val) {
  auto parts = split_ws(*args);
  const std::string ne = name + "=";
  for (size_t i = 0; i < parts.size(); i++) {
    if (parts[i].compare(0, ne.size(), ne) == 0) {
      *val = parts[i].substr(ne.size());
      std::string rest;
      for (size_t j = 0; j < parts.size(); j++)
        if (j != i) rest += (rest.empty() ? "" : " ") + parts[j];
      *args = rest;
      return true;
    }
  }
  return false;
}
inline bool ParseFromString(const std::string &name, std::string *args, int *v) {
  std::string s;
  if (!take(name, args, &s)) return false;
  char *end = nullptr;
  long x = strtol(s.c_str(), &end, 10);
  if (s.empty() || *end) throw std::invalid_argument("Bad option " + name + "=" + s);
  *v = (int)x;
  return true;
}
inline bool ParseFromString(const std::string &name, std::string *args, float *v) {
  std::string s;
  if (!take(name, args, &s)) return false;
  char *end = nullptr;
  double x = strtod(s.c_str(), &end);
  if (s.empty() || *end) throw std::invalid_argument("Bad option " + name + "=" + s);
  *v = (float)x;
  return true;
}
inline bool ParseFromString(const std::string &name, std::string *args, bool *v) {
  std::string s;
  if (!take(name, args, &s)) return false;
  if (s.empty()) throw std::invalid_argument("Bad option " + name);
  if (s[0] == 'f' || s[0] == 'F') *v = false;
  else if (s[0] == 't' || s[0] == 'T') *v = true;
  else throw std::invalid_argument("Bad option " + name + "=" + s);
  return true;
}
inline bool ParseFromString(const std::string &name, std::string *args, std::vector<int> *v) {
  std::string s;
  if (!take(name, args, &s)) return false;
  v->clear();
  std::stringstream ss(s);
  std::string tok;
  while (std::getline(ss, tok, ':')) v->push_back(std::stoi(tok));
  return true;
}

// ---- Kaldi token stream, both modes (kaldi_io.h) ----
using kio::ExpectToken;
using kio::WriteToken;
// counters are int32 in the reference's files (nnet-cudnn-component.h:263-266)
inline int32_t as_i32(double v) { return (int32_t)(uint32_t)(uint64_t)(int64_t)v; }
inline std::vector<float> d2h(const float *d, long n) {
  std::vector<float> h((size_t)n);
  if (n) {
    KCTC_HIP_CHECK(hipMemcpyAsync(h.data(), d, sizeof(float) * n, hipMemcpyDeviceToHost, S()));
    KCTC_HIP_CHECK(hipStreamSynchronize(S()));
  }
  return h;
}
inline void h2d(float *d, const float *h, long n) {
  if (!n) return;
  KCTC_HIP_CHECK(hipMemcpyAsync(d, h, sizeof(float) * n, hipMemcpyHostToDevice, S()));
  KCTC_HIP_CHECK(hipStreamSynchronize(S()));
}

}  // namespace nnet2
}  // namespace kctc
