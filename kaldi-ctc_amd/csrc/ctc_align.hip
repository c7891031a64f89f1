// ctc_align.hip -- CTC forced alignment (Viterbi) for MI355X (gfx950): the
// best path through the blank-interleaved label sequence of a given
// transcript, per utterance (include/ctc.h, extensions).
//
// Three launches per call, all stream-ordered:
//   K1 ctc_logz       ctc.hip's per-frame normaliser: lp = act - logsumexp(act).
//   K2 ctc_viterbi    one workgroup per utterance, serial over T: the alpha
//                     recursion of ctc.hip's long-label kernel with max in
//                     place of the log-sum-exp.  Thread `tid` owns the states
//                     tid + i * blockDim.x: one state per thread in up to 8
//                     waves (S <= 512), else 512 threads and 3 states per
//                     thread.  Extended labels in registers, emissions
//                     gathered into LDS a chunk of frames ahead by LDS-DMA,
//                     the previous column in double-buffered LDS, one LDS-only
//                     barrier per frame.  Every column is renormalised by the
//                     previous column's max (the same number for every state,
//                     so ties stay ties) with the running offset in fp64.
//                     Back-pointers (0 stay, 1 step, 2 skip) leave as two
//                     64-bit ballots per wave and 64-state block: 2 bits per
//                     state, one 16-byte store per wave and block.
//   K3 ctc_backtrace  one workgroup per utterance: chunks of 64 frames from
//                     the end.  A chunk moves the state by at most 126, so the
//                     back-pointer words of 3 state blocks per frame are
//                     staged into LDS by the whole workgroup and one lane
//                     chases them there; the workgroup then writes the chunk's
//                     ids.  Also fills the padding rows with -1.
// Deterministic: no atomics, a fixed order everywhere.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>

#include "common.h"
#include "ctc.h"
#include "ctc_shared.h"
#include "prof.h"

namespace kctc {
namespace ctcimpl {

constexpr int kVitThreads = 512;  // the 3-states-per-thread kernel
constexpr int kVitWaves = kVitThreads / 64;
constexpr int kVitSPT = (2 * kMaxLabel + 1 + kVitThreads - 1) / kVitThreads;  // 3
constexpr int kBtThreads = 256;
constexpr int kBtF = 64;   // frames per backtrace chunk
constexpr int kBtNB = 3;   // 64-state blocks a chunk's window can touch: 2 (kBtF - 1) + 1 states

typedef unsigned long long u64;
struct BpWord { u64 lo, hi; };  // bit j: bit 0 / bit 1 of the back-pointer of state 64 b + j
static_assert(sizeof(BpWord) == 16, "one 16-byte store");

struct AlignLayout {
  size_t desc, labels, send, logz, lp, bp, total;
  int T_max, L_max;
  long long nlab;
};

// Checks the lengths and lays the workspace out; false: invalid lengths.
static bool make_align_layout(const int *label_lengths, const int *input_lengths, int A, int N, AlignLayout *lay,
                              std::vector<UttDesc> *descs) {
  if (A <= 0 || N <= 0 || !label_lengths || !input_lengths) return false;
  int T_max = 0, L_max = 0;
  long long nlab = 0, words = 0;
  if (descs) descs->resize(N);
  for (int n = 0; n < N; n++) {
    const int T = input_lengths[n], L = label_lengths[n];
    if (T < 0 || L < 0 || L > kMaxLabel) return false;
    T_max = std::max(T_max, T);
    L_max = std::max(L_max, L);
    const int S = 2 * L + 1;
    if (descs) {
      UttDesc &d = (*descs)[n];
      d.T = T; d.L = L; d.S = S; d.feasible = 0; d.lab_off = (int)nlab; d.pad = 0;
      d.ab_off = words; d.off_off = 0;
    }
    nlab += L;
    words += (long long)T * ((S + 63) / 64);  // frame 0 has no back-pointer: its row is never touched
  }
  AlignLayout &l = *lay;
  size_t p = 0;
  l.desc = p;   p = align_up(p + sizeof(UttDesc) * N, 256);
  l.labels = p; p = align_up(p + sizeof(int) * (nlab > 0 ? nlab : 1), 256);
  l.send = p;   p = align_up(p + sizeof(int) * N, 256);  // end state of each utterance (-1: infeasible)
  l.logz = p;   p = align_up(p + sizeof(float) * (size_t)T_max * N + 4, 256);
  l.lp = p;     p = align_up(p + sizeof(float) * (size_t)T_max * N * A + 4, 256);
  l.bp = p;     p = align_up(p + sizeof(BpWord) * (size_t)words, 256);
  l.total = p;
  l.T_max = T_max;
  l.L_max = L_max;
  l.nlab = nlab;
  return true;
}

// dynamic LDS of K2, one array as in ctc.hip: emit[2][F][SP] | col[2][CP] | wmax[2][kVitWaves]
struct VitLds {
  int F, SP, CP;
  size_t floats() const { return 2 * (size_t)F * SP + 2 * (size_t)CP + 2 * kVitWaves + 4; }
};

// ---------------------------------------------------------------------------
// K2: v_t(s) = lp[t][l'_s] + max(v_{t-1}(s), v_{t-1}(s-1), v_{t-1}(s-2)), the
// last only where the skip is allowed; a later candidate wins only if it is
// strictly greater.  blockDim.x = 64 x waves, SPT states per thread.
// ---------------------------------------------------------------------------
template <int SPT>
__global__ __launch_bounds__(kVitThreads) void ctc_viterbi(
    const float *__restrict__ lp, int N, int A, int blank, const UttDesc *__restrict__ descs,
    const int *__restrict__ labels, BpWord *__restrict__ bp, int *__restrict__ s_end,
    double *__restrict__ scores, VitLds lay) {
  const int n = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nthr = blockDim.x, nwv = nthr >> 6;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int F = lay.F, SP = lay.SP, CP = lay.CP;
  float *emit = lds;                        // [2][F][SP]
  float *colb = emit + 2 * (size_t)F * SP;  // [2][CP]
  float *wmax = colb + 2 * CP;              // [2][kVitWaves]

  const UttDesc d = descs[n];
  const int T = d.T, S = d.S;
  if (!d.feasible) {  // workgroup-uniform
    if (tid == 0) {
      scores[n] = -INFINITY;
      s_end[n] = -1;
    }
    return;
  }
  const int *lab = labels + d.lab_off;

  // extended label of each owned state s = tid + nthr i, and its skip permission
  int ext[SPT];
  bool skip[SPT];
#pragma unroll
  for (int i = 0; i < SPT; i++) {
    const int s = tid + i * nthr;
    ext[i] = (s < S && (s & 1)) ? lab[(s - 1) >> 1] : blank;
    skip[i] = s < S && (s & 1) && s >= 2 && lab[(s - 1) >> 1] != lab[(s - 3) >> 1];
  }

  const long tstride = (long)N * A;
  const float *lrow = lp + (long)n * A;  // + t * N * A
  const int nblk = (S + 63) / 64;        // 64-state blocks; wave w owns blocks w, w + nwv, ...
  BpWord *bpu = bp + d.ab_off;           // [T][nblk]
  auto issue = [&](int c, int b) {
    float *dst = emit + (size_t)b * F * SP;
    for (int f = 0; f < F; f++) {
      const int t = c * F + f;
      if (t >= T) break;
      const float *src = lrow + (long)t * tstride;
#pragma unroll
      for (int i = 0; i < SPT; i++) {
        const int sb = wid + nwv * i;
        if (sb < nblk) __builtin_amdgcn_global_load_lds(src + ext[i], dst + (size_t)f * SP + sb * 64, 4, 0, 0);
      }
    }
  };

  if (tid < 2 * kVitWaves) wmax[tid] = -INFINITY;  // a launch of fewer waves never writes the rest
  issue(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  lds_barrier();
  double off = 0.0;
  int cur = 0;
  const int nchunk = (T + F - 1) / F;
  for (int c = 0; c < nchunk; c++) {
    if (c + 1 < nchunk) issue(c + 1, (c + 1) & 1);
    const float *em = emit + (size_t)(c & 1) * F * SP;
    const int fend = min(F, T - c * F);
    for (int f = 0; f < fend; f++) {
      const int t = c * F + f;
      float ly[SPT];
#pragma unroll
      for (int i = 0; i < SPT; i++) ly[i] = em[(size_t)f * SP + min(tid + i * nthr, SP - 1)];
      float *cc = colb + cur * CP;
      float lmax = -INFINITY;
      if (t == 0) {
#pragma unroll
        for (int i = 0; i < SPT; i++) {
          const int s = tid + i * nthr;
          const float q = (s <= 1 && s < S) ? ly[i] : -INFINITY;
          cc[s] = q;
          lmax = fmaxf(lmax, q);
        }
      } else {
        // all LDS reads of the frame up front, branch-free (clamped indices,
        // -inf selected in); cc holds SPT * nthr entries, so every lane
        // computes and writes and the states >= S only ever feed selects
        const float *wm = wmax + (cur ^ 1) * kVitWaves;
        const float *pv = colb + (cur ^ 1) * CP;
        float pa[SPT], pb[SPT], pc[SPT];
#pragma unroll
        for (int i = 0; i < SPT; i++) {
          const int s = tid + i * nthr;
          pa[i] = pv[s];
          pb[i] = pv[max(s - 1, 0)];
          pc[i] = pv[max(s - 2, 0)];
          pb[i] = s >= 1 ? pb[i] : -INFINITY;
          pc[i] = skip[i] ? pc[i] : -INFINITY;
        }
        // all kVitWaves entries, unrolled: the reads issue together and share
        // one wait (the entries of waves that do not exist stay -inf)
        float mu = wm[0];
#pragma unroll
        for (int w = 1; w < kVitWaves; w++) mu = fmaxf(mu, wm[w]);
#pragma unroll
        for (int i = 0; i < SPT; i++) {
          const int s = tid + i * nthr;
          float best = pa[i];
          int b = 0;
          if (pb[i] > best) { best = pb[i]; b = 1; }
          if (pc[i] > best) { best = pc[i]; b = 2; }
          const float q = (best - mu) + ly[i];
          cc[s] = q;
          lmax = fmaxf(lmax, s < S ? q : -INFINITY);
          // 2 bits per state: the wave's 64 low bits, then its 64 high bits
          const u64 lo = __builtin_amdgcn_ballot_w64((b & 1) != 0);
          const u64 hi = __builtin_amdgcn_ballot_w64((b & 2) != 0);
          const int sb = wid + nwv * i;
          if (lane == 0 && sb < nblk) bpu[(long)t * nblk + sb] = BpWord{lo, hi};
        }
        off += (double)mu;
      }
      lmax = wave_max_l63(lmax);
      if (lane == 63) wmax[cur * kVitWaves + wid] = lmax;
      lds_barrier();
      cur ^= 1;
    }
    // the next chunk's gathers have landed; every wave is done with this chunk's buffer
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    lds_barrier();
  }
  if (tid == 0) {
    // the best path ends in the last blank or the last label; the label only
    // if it is strictly better
    const float *pv = colb + (cur ^ 1) * CP;
    const float a = pv[S - 1], b = S > 1 ? pv[S - 2] : -INFINITY;
    const bool label_end = S > 1 && b > a;
    s_end[n] = label_end ? S - 2 : S - 1;
    scores[n] = off + (double)(label_end ? b : a);
  }
}

// ---------------------------------------------------------------------------
// K3: s_{t-1} = s_t - bp_t(s_t), ali[t] = l'_{s_t}; rows t >= T get -1.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBtThreads) void ctc_backtrace(
    const UttDesc *__restrict__ descs, const int *__restrict__ labels, const BpWord *__restrict__ bp,
    const int *__restrict__ s_end, int N, int T_max, int blank, int *__restrict__ ali) {
  __shared__ BpWord win[kBtF][kBtNB];
  __shared__ int path[kBtF];
  __shared__ int s_next;
  const int n = blockIdx.x, tid = threadIdx.x;
  const UttDesc d = descs[n];
  int s = s_end[n];
  const int T = s >= 0 ? d.T : 0;  // infeasible: every row is padding
  for (int t = T + tid; t < T_max; t += kBtThreads) ali[(long)t * N + n] = -1;
  if (T == 0) return;
  const int nblk = (d.S + 63) / 64;
  const BpWord *bpu = bp + d.ab_off;
  const int *lab = labels + d.lab_off;
  for (int thi = T - 1; thi >= 0; thi -= kBtF) {
    const int nf = min(kBtF, thi + 1);  // frames thi, thi - 1, ..., thi - nf + 1
    // frame thi - f is in a state of [s - 2 f, s]: blocks b0 .. b0 + kBtNB - 1
    const int b0 = max(s - 2 * (kBtF - 1), 0) >> 6;
    for (int it = tid; it < nf * kBtNB; it += kBtThreads) {
      const int f = it / kBtNB, j = it - f * kBtNB, t = thi - f;
      if (t >= 1 && b0 + j < nblk) win[f][j] = bpu[(long)t * nblk + b0 + j];
    }
    __syncthreads();
    if (tid == 0) {
      int sc = s;
      for (int f = 0; f < nf; f++) {
        path[f] = sc;
        if (thi - f >= 1) {
          const BpWord w = win[f][(sc >> 6) - b0];
          const int bit = sc & 63;
          sc -= (int)((w.lo >> bit) & 1) | ((int)((w.hi >> bit) & 1) << 1);
        }
      }
      s_next = sc;
    }
    __syncthreads();
    for (int f = tid; f < nf; f += kBtThreads) {
      const int sc = path[f];
      ali[(long)(thi - f) * N + n] = (sc & 1) ? lab[(sc - 1) >> 1] : blank;
    }
    s = s_next;
    __syncthreads();  // win, path and s_next are rewritten by the next chunk
  }
}

// 0: the 3-states-per-thread kernel for every batch (mictc_set_align_kernel, for the tests)
static std::atomic<int> g_small{1};

static ctcStatus_t launch_align(const AlignLayout &lay, std::vector<UttDesc> &descs, const float *acts,
                                const int *flat_labels, const int *label_lengths, int A, int N, int *ali_dev,
                                double *scores_dev, void *workspace, hipStream_t stream, int blank) {
  if (blank < 0 || blank >= A || !acts || !workspace || !ali_dev || !scores_dev) return CTC_STATUS_INVALID_VALUE;
  const long long nlab = lay.nlab;
  if (nlab && !flat_labels) return CTC_STATUS_INVALID_VALUE;
  for (long long i = 0; i < nlab; i++)
    if (flat_labels[i] < 0 || flat_labels[i] >= A || flat_labels[i] == blank) return CTC_STATUS_INVALID_VALUE;
  // feasible: T > 0 and L + repeats <= T (the loss kernel's rule)
  for (int n = 0; n < N; n++) {
    UttDesc &d = descs[n];
    const int *lab = flat_labels + d.lab_off;
    int rep = 0;
    for (int i = 1; i < d.L; i++) rep += lab[i] == lab[i - 1];
    d.feasible = d.T > 0 && d.L + rep <= d.T;
  }
  char *ws = static_cast<char *>(workspace);
  // descriptors then labels: one H2D copy from the pinned staging buffer
  char *stage = staging_acquire(lay.send);
  if (!stage) return CTC_STATUS_MEMOPS_FAILED;
  memcpy(stage + lay.desc, descs.data(), sizeof(UttDesc) * N);
  if (nlab) memcpy(stage + lay.labels, flat_labels, sizeof(int) * nlab);
  if (hipMemcpyAsync(ws, stage, lay.send, hipMemcpyHostToDevice, stream) != hipSuccess)
    return CTC_STATUS_MEMOPS_FAILED;
  staging_release(stream);
  const UttDesc *d_desc = reinterpret_cast<const UttDesc *>(ws + lay.desc);
  const int *d_lab = reinterpret_cast<const int *>(ws + lay.labels);
  int *d_send = reinterpret_cast<int *>(ws + lay.send);
  float *d_lp = reinterpret_cast<float *>(ws + lay.lp);
  BpWord *d_bp = reinterpret_cast<BpWord *>(ws + lay.bp);
  const long rows = (long)lay.T_max * N;
  if (rows > 0) launch_logz(acts, A, rows, reinterpret_cast<float *>(ws + lay.logz), d_lp, stream);

  const int Smax = 2 * lay.L_max + 1;
  const bool small = Smax <= kVitThreads && g_small.load(std::memory_order_relaxed) != 0;
  const int nthr = small ? (Smax + 63) / 64 * 64 : kVitThreads;
  VitLds vl;
  vl.SP = (Smax + 63) / 64 * 64;
  vl.CP = (small ? 1 : kVitSPT) * nthr + 4;  // every owned state of every thread is written
  // chunk depth: as many frames as fit 96 KB of double-buffered emissions (4..32)
  vl.F = (int)std::min<size_t>(32, std::max<size_t>(4, (size_t)96 * 1024 / (2 * sizeof(float) * vl.SP)));
  const size_t shm = sizeof(float) * vl.floats();
  if (shm > 160 * 1024) return CTC_STATUS_INVALID_VALUE;
  {
    const auto kern = small ? ctc_viterbi<1> : ctc_viterbi<kVitSPT>;
    ProfSpan ps(stream, "ctc_viterbi");
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)shm);
    hipLaunchKernelGGL(kern, dim3(N), dim3(nthr), shm, stream, d_lp, N, A, blank, d_desc, d_lab, d_bp, d_send,
                       scores_dev, vl);
  }
  {
    ProfSpan ps(stream, "ctc_backtrace");
    hipLaunchKernelGGL(ctc_backtrace, dim3(N), dim3(kBtThreads), 0, stream, d_desc, d_lab, d_bp, d_send, N,
                       lay.T_max, blank, ali_dev);
  }
  if (hipGetLastError() != hipSuccess) return CTC_STATUS_EXECUTION_FAILED;
  return CTC_STATUS_SUCCESS;
}

}  // namespace ctcimpl
}  // namespace kctc

using namespace kctc::ctcimpl;

extern "C" {

int mictc_set_align_kernel(int on) {
  const int prev = g_small.load();
  if (on >= 0) g_small.store(on ? 1 : 0);
  return prev;
}

ctcStatus_t mictc_get_align_workspace_size(const int *label_lengths, const int *input_lengths, int alphabet_size,
                                           int minibatch, size_t *size_bytes) {
  if (!size_bytes) return CTC_STATUS_INVALID_VALUE;
  AlignLayout lay;
  if (!make_align_layout(label_lengths, input_lengths, alphabet_size, minibatch, &lay, nullptr))
    return CTC_STATUS_INVALID_VALUE;
  *size_bytes = lay.total;
  return CTC_STATUS_SUCCESS;
}

ctcStatus_t mictc_ctc_align_async(const float *activations, const int *flat_labels, const int *label_lengths,
                                  const int *input_lengths, int alphabet_size, int minibatch, int *ali_dev,
                                  double *scores_dev, void *workspace, ctcStream_t stream, int blank_label) {
  try {
    AlignLayout lay;
    std::vector<UttDesc> descs;
    if (!make_align_layout(label_lengths, input_lengths, alphabet_size, minibatch, &lay, &descs))
      return CTC_STATUS_INVALID_VALUE;
    return launch_align(lay, descs, activations, flat_labels, label_lengths, alphabet_size, minibatch, ali_dev,
                        scores_dev, workspace, reinterpret_cast<hipStream_t>(stream), blank_label);
  } catch (...) {
    return CTC_STATUS_UNKNOWN_ERROR;
  }
}

}  // extern "C"
