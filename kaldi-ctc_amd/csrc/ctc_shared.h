// ctc_shared.h -- what the CTC loss (ctc.hip), the CTC forced alignment
// (ctc_align.hip) and the CTC prefix beam search (ctc_beam.hip) share: the
// utterance descriptor, the LDS-only barrier of the
// serial frame loops, the per-frame normaliser's launch and the pinned staging
// buffer of the host arrays.  Private to csrc/.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace kctc {
namespace ctcimpl {

constexpr int kMaxLabel = 639;  // MAX_WARPCTC_LABEL_LENGTH, src/ctc/ctc-nnet-train.cc:25-26

struct UttDesc {
  int T, L, S, feasible, lab_off, pad;
  long long ab_off;   // loss: float offset of this utterance's alpha spill; beta follows at +T*S
                      // alignment: offset, in 16-byte words, of its back-pointer spill
                      // beam search: offset, in 16-byte nodes, of its prefix node pool
  long long off_off;  // loss: double offset of offA[T]; offB follows at +T (alignment: unused)
};

// waits for this wave's LDS traffic only, then the workgroup barrier (a
// __syncthreads() would also drain the LDS-DMA in flight)
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// K1 of ctc.hip, ProfSpan "ctc_logz": logz[row] = logsumexp_a acts[row][a] and
// lp[row][a] = acts[row][a] - logz[row], one wave per row (ctc.hip)
void launch_logz(const float *acts, int A, long rows, float *logz, float *lp, hipStream_t stream);

// Pinned host staging of the calling thread, reused once the previous call's
// copy has landed (ctc.hip): acquire waits for that copy and returns at least
// `bytes` (nullptr: a HIP call failed); release marks the buffer busy until
// the work queued so far on `stream` is done.
char *staging_acquire(size_t bytes);
void staging_release(hipStream_t stream);

}  // namespace ctcimpl
}  // namespace kctc
