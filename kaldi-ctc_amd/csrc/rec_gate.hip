// rec_gate.hip -- residency of the v6 recurrences: the launches beside a
// running recurrence (rnn.h rnn_side_gated), the residency gate of the
// gradient exchange (rnn.h rnn_comm_gate) and the epoch gate of the streamed
// weight gradients.
#include <algorithm>
#include <stdexcept>

#include "common.h"
#include "rec_gate.h"

namespace kctc {

// ---- launches beside a running recurrence (rnn.h rnn_side_gated) ----
namespace {
// the v6 recurrence this host thread enqueued last, while the host function
// that enqueued it runs (RecScope), and the side streams gated on it
struct RecInFlight {
  const unsigned *res = nullptr;    // its residency word (p.flags + kResWord)
  const unsigned *flags = nullptr;  // its flag area
  unsigned target = 0;              // its workgroups
  hipStream_t gated[4] = {};
  int ngated = 0;
};
thread_local RecInFlight g_rec;
}  // namespace

void RecScope::enqueued(unsigned *flags, int workgroups) {
  g_rec = RecInFlight{};
  g_rec.res = flags + kResWord;
  g_rec.flags = flags;
  g_rec.target = (unsigned)workgroups;
}
void RecScope::none() { g_rec = RecInFlight{}; }

void beside_recurrence(hipStream_t side) {
  if (!g_rec.res) throw std::logic_error("beside_recurrence: no recurrence in flight");
  for (int i = 0; i < g_rec.ngated; i++)
    if (g_rec.gated[i] == side) return;  // (already behind this recurrence's gate)
  if (g_rec.ngated == 4) throw std::logic_error("beside_recurrence: too many side streams");
  rnn_resident_gate(side, g_rec.flags, g_rec.target);
  g_rec.gated[g_rec.ngated++] = side;
}

bool rnn_side_gated(hipStream_t s) {
  if (!g_rec.res) return true;
  for (int i = 0; i < g_rec.ngated; i++)
    if (g_rec.gated[i] == s) return true;
  return false;
}

// ---- residency gate of the gradient exchange (rnn.h) ----
namespace {
RegWord g_reg[64];
int g_comm_gated[64] = {0};  // per device: live gated exchanges (at most one, GatedExchange)
int current_device() {
  int dev = 0;
  KCTC_HIP_CHECK(hipGetDevice(&dev));
  return dev & 63;
}
}  // namespace
RegWord &reg_of_device() {
  int dev = 0;
  KCTC_HIP_CHECK(hipGetDevice(&dev));
  RegWord &r = g_reg[dev & 63];
  if (!r.word) {
    KCTC_HIP_CHECK(hipMalloc(&r.word, 256));
    KCTC_HIP_CHECK(hipMemset(r.word, 0, 256));
  }
  return r;
}

// The gates poll the word (10 s at most, then they give up and set bit 0 of
// the device word's [1]).  hipStreamWaitValue is no alternative: ROCclr runs
// it as a one-thread kernel too (__amd_rocclr_streamOpsWait), without a
// timeout -- under rocprofv3's counter collection, which serialises
// dispatches, a gate dispatched before its recurrence then never returns.
// A gate is kGateBlocks one-wave blocks, one per XCD (round-robin dispatch).
// A wave of it holds a CU, and a recurrence workgroup that needs a CU's whole
// register file (configs[4]'s bf16 GRU backward: 256 VGPRs x 2 waves per
// SIMD) cannot be placed beside it: a gate on one of the 32 CUs of an XCD the
// recurrence is pinned to kept that XCD's last workgroup out until the gate
// timed out (error 0x10003 at configs[4] with KCTC_STREAM_ALL=1).  So a block
// leaves as soon as the recurrence has a workgroup on its own XCD (xw: the
// XCD bits its workgroups OR in first thing), unless it is the last block
// still waiting (leave counts the ones gone): the blocks on XCDs the
// recurrence does not use do the waiting.  (A full-register recurrence on all
// eight XCDs would keep the last block's CU; no recipe shape is one -- with
// every CU taken nothing streams beside it either -- and the gate's timeout
// would flag it.)
constexpr int kGateBlocks = 8;
template <typename W>
__global__ __launch_bounds__(64) void gate_kernel(const W *word, W target, unsigned *gerr, const unsigned *xw,
                                                  unsigned *leave) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  const unsigned me = 1u << xcc_id();
  bool late = false;
  while (true) {
    const W v = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (__builtin_amdgcn_readfirstlane((int)(v >= target))) break;
    if (xw && __builtin_amdgcn_readfirstlane((int)(__hip_atomic_load(xw, __ATOMIC_RELAXED,
                                                                     __HIP_MEMORY_SCOPE_AGENT) & me))) {
      unsigned gone = 0;
      if (threadIdx.x == 0) gone = atomicAdd(leave, 1u);
      if (__builtin_amdgcn_readfirstlane((int)gone) < kGateBlocks - 1) return;
      xw = nullptr;  // the last one: it stays
    }
    late = __builtin_amdgcn_s_memrealtime() - t0 > 1000000000ull;  // 100 MHz clock
    if (late) break;
    __builtin_amdgcn_s_sleep(8);
  }
  if (late && threadIdx.x == 0) atomicOr(gerr, 1u);
}

unsigned long long rnn_bwd_registrations() { return reg_of_device().expected; }
void rnn_resident_gate(hipStream_t s, const unsigned *flags, unsigned target) {
  hipLaunchKernelGGL(gate_kernel<unsigned>, dim3(kGateBlocks), dim3(64), 0, s, flags + kResWord, target,
                     reg_of_device().word + 1, flags + kXcdWord, const_cast<unsigned *>(flags) + kGateWord);
  KCTC_HIP_CHECK(hipGetLastError());
}
const unsigned *rnn_pinned_xcds() { return reg_of_device().word + 2; }

void rnn_comm_gate(hipStream_t s, unsigned long long target) {
  RegWord &r = reg_of_device();
  // XCDs of the pinned backward recurrences (word [2], never cleared); the
  // blocks gone counted in word [6], zeroed per gate on its own stream
  KCTC_HIP_CHECK(hipMemsetAsync(r.word + 6, 0, sizeof(unsigned), s));
  hipLaunchKernelGGL(gate_kernel<unsigned long long>, dim3(kGateBlocks), dim3(64), 0, s,
                     reinterpret_cast<const unsigned long long *>(r.word + 4), target, r.word + 1, r.word + 2,
                     r.word + 6);
  KCTC_HIP_CHECK(hipGetLastError());
}
void rnn_set_comm_gated(bool on) {
  int &c = g_comm_gated[current_device()];
  c = on ? c + 1 : std::max(0, c - 1);
}
bool rnn_comm_gated() { return g_comm_gated[current_device()] > 0; }

// ---- epoch gate of the streamed weight gradients (rnn.h RnnWgradStream) ----
namespace {
// One wave: returns once every v6 flag line (stride kFlagStride words) holds
// >= epoch, the recurrence reported an error, or after 3 s (then err bit 3).
// Every exit decision is wave-uniform; the error store follows the loop.
__global__ __launch_bounds__(64) void rec_gate_kernel(const unsigned *flags, int nlines, unsigned epoch,
                                                      unsigned *err) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  int spins = 0;
  bool late = false;
  while (true) {
    bool ok = true;
    for (int i = threadIdx.x; i < nlines; i += 64)
      ok &= __hip_atomic_load(flags + (long)i * kFlagStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= epoch;
    if (__all(ok)) break;
    if ((++spins & 255) == 0) {
      const unsigned e = __builtin_amdgcn_readfirstlane(__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      if (e) break;
      late = __builtin_amdgcn_s_memrealtime() - t0 > 300000000ull;
      if (late) break;
    }
    __builtin_amdgcn_s_sleep(16);
  }
  if (late && threadIdx.x == 0) atomicOr(err, 8u);
}
}  // namespace
void rec_epoch_gate(hipStream_t s, const unsigned *lines, int nlines, unsigned epoch, unsigned *err) {
  hipLaunchKernelGGL(rec_gate_kernel, dim3(1), dim3(64), 0, s, lines, nlines, epoch, err);
}

}  // namespace kctc
