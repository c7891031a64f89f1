// cu_device.cpp -- device buffers and the per-thread device context of nnet.h:
// DevBuf, CuMatrix, CuDevice (streams, fork / join, profiling spans), Rng.
#include <algorithm>

#include "common.h"
#include "nnet.h"
#include "prof.h"

namespace kctc {
namespace nnet2 {

DevBuf::~DevBuf() {
  if (p) (void)hipFree(p);
}

void DevBuf::ensure(size_t b) {
  if (b <= bytes && p) return;
  if (p) {
    auto &d = CuDevice::Instantiate();
    KCTC_HIP_CHECK(hipStreamSynchronize(d.stream));
    if (d.side) KCTC_HIP_CHECK(hipStreamSynchronize(d.side));
    if (d.stream2) KCTC_HIP_CHECK(hipStreamSynchronize(d.stream2));
    KCTC_HIP_CHECK(hipFree(p));
    p = nullptr;
  }
  size_t nb = align_up(std::max<size_t>(b, 256), 4096);
  KCTC_HIP_CHECK(hipMalloc(&p, nb));
  // zeroed before any use (flag words that hold ids, e.g. the gated
  // projection's tile flags, must not start out as one by chance)
  KCTC_HIP_CHECK(hipMemsetAsync(p, 0, nb, nullptr));
  KCTC_HIP_CHECK(hipStreamSynchronize(nullptr));
  bytes = nb;
}

void CuMatrix::Resize(long rows, int cols) {
  buf_.ensure(sizeof(float) * (size_t)std::max<long>(1, rows * (long)cols));
  data_ = buf_.f();
  rows_ = rows;
  cols_ = cols;
}

CuDevice &CuDevice::Instantiate() {
  static thread_local CuDevice dev;
  return dev;
}

void CuDevice::Fork() {
  if (!side) return;
  if (!fork_ev) KCTC_HIP_CHECK(hipEventCreateWithFlags(&fork_ev, hipEventDisableTiming));
  KCTC_HIP_CHECK(hipEventRecord(fork_ev, stream));
  KCTC_HIP_CHECK(hipStreamWaitEvent(side, fork_ev, 0));
}

void CuDevice::Join() {
  if (!side) return;
  if (!join_ev) KCTC_HIP_CHECK(hipEventCreateWithFlags(&join_ev, hipEventDisableTiming));
  KCTC_HIP_CHECK(hipEventRecord(join_ev, side));
  KCTC_HIP_CHECK(hipStreamWaitEvent(stream, join_ev, 0));
}

void CuDevice::Begin(const char *family, hipStream_t s) {
  if (!profiling) return;
  if (!s) s = stream;
  if (pool.size() < 2) {
    for (int i = 0; i < 64; i++) {
      hipEvent_t e;
      KCTC_HIP_CHECK(hipEventCreate(&e));
      pool.push_back(e);
    }
  }
  Span sp;
  sp.family = family;
  sp.a = pool.back(); pool.pop_back();
  sp.b = pool.back(); pool.pop_back();
  sp.s = s;
  KCTC_HIP_CHECK(hipEventRecord(sp.a, s));
  open.push_back(spans.size());
  spans.push_back(sp);
}

void CuDevice::End() {
  if (!profiling || open.empty()) return;
  KCTC_HIP_CHECK(hipEventRecord(spans[open.back()].b, spans[open.back()].s));
  open.pop_back();
}

void CuDevice::Collect() {
  for (auto &sp : spans) {
    float ms = 0.f;
    KCTC_HIP_CHECK(hipEventElapsedTime(&ms, sp.a, sp.b));
    auto &e = prof[sp.family];
    e.first += ms;
    e.second += 1;
    pool.push_back(sp.a);
    pool.push_back(sp.b);
  }
  spans.clear();
}

}  // namespace nnet2

void prof_begin(hipStream_t s, const char *family) {
  auto &d = nnet2::CuDevice::Instantiate();
  if (d.profiling && (s == d.stream || (s && s == d.side))) d.Begin(family, s);
}
void prof_end(hipStream_t s) {
  auto &d = nnet2::CuDevice::Instantiate();
  if (d.profiling && (s == d.stream || (s && s == d.side))) d.End();
}

namespace nnet2 {

uint64_t Rng::next() {
  uint64_t z = (s += 0x9E3779B97F4A7C15ULL);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}
double Rng::uniform() { return ((double)(next() >> 11) + 0.5) * (1.0 / 9007199254740992.0); }
double Rng::gauss() {
  const double u1 = uniform(), u2 = uniform();
  return std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2);
}

}  // namespace nnet2
}  // namespace kctc
