// rec_common.h -- what the recurrence kernels (rec_generic.hip: the generic
// pair, rec6_fwd.hip, rec6_bwd.hip: v6) and their host (rnn.hip, rnn_plan.hip,
// rec_gate.hip) share: RecParams,
// the hand-off helpers, trace stamps, the named flag words; V6Cfg and the
// kernel lookups.  The unnamed namespace's contents are per translation unit.
#pragma once
#include <stdexcept>

#include "common.h"
#include "rnn.h"

namespace kctc {

// The template argument P a v6 launch runs with (pick6 decides): plain
// (kPrecX3 / kPrecBf16), stacked (kPrecX3S: hi / lo of a <= 8-row group in one
// MFMA operand) or IO-wave (P | 4, forward only: the upper waves fetch G)
enum Rec6Variant { kRec6None = 0, kRec6Plain = 1, kRec6Stacked = 2, kRec6IoWave = 3 };
// One v6 configuration of a (descriptor, N, direction of time): pick6 (rnn_plan.hip)
struct V6Cfg {
  int U = 0, nth = 0, rg = 0, gs = 16, variant = kRec6None;
  explicit operator bool() const { return U > 0; }
};
// The __global__ function of a recurrence (to launch, or to ask for its
// attributes); std::logic_error for a shape that is not compiled.  Generic:
// rt = 16-row tiles of the batch.
const void *rec6_fwd_kernel(int mode, int prec, int H, const V6Cfg &c);
const void *rec6_bwd_kernel(int mode, int prec, int H, const V6Cfg &c);
const void *rec_generic_kernel(bool fwd, int mode, int rt);
inline const void *rec6_kernel(bool fwd, int mode, int prec, int H, const V6Cfg &c) {
  return fwd ? rec6_fwd_kernel(mode, prec, H, c) : rec6_bwd_kernel(mode, prec, H, c);
}

namespace {

constexpr int NT = 256;
constexpr int kSpinLimit = 1 << 21;
constexpr int kMaxRT = 4;  // N <= 64 (four 16-row MFMA tiles)
constexpr int kMaxCT = 4;  // <= 64 gate columns per workgroup

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void *base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, bytes, 0x00020000);
}

__device__ __forceinline__ u32x4 ld_sc1(__amdgpu_buffer_rsrc_t r, unsigned off) {
  return __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 16 /* sc1 */);
}

struct RecParams {
  int T, N, H, dirs, U, nwg, ncol, Npad;
  int rg;           // v6: row groups (independent recurrences) of gs sequences
  int gs;           // v6: sequences per row group (16, or 8: two groups of a 16-row batch run side by side)
  const float *w;   // params base of this stacked layer's pseudo-layer 0
  long pl_stride;   // floats between the two directions' blocks
  long r_off;       // R within a pseudo-layer block
  long bR_off;      // bR within a pseudo-layer block
  float *G;         // [T*N][dirs*nW*H] pre-activations -> activations
  float *y;         // [T*N][dirs*H] output
  float *aux;       // LSTM: c ; GRU: R_n h + b_Rn   [T*N][dirs*H]
  const float *dy;  // backward: [T*N][dirs*H]
  float *E;         // backward: dGates (recurrent part) [T*N][dirs*nW*H]
  float *DX;        // backward GRU: dGates (input part); == E otherwise
  float *bias;      // backward: bias partial sums [dirs][2][nW*H]
  unsigned *flags;  // generic: [dirs][nwg] step epochs; v6: flag6; zeroed before launch
  unsigned *err;
  // unused: the place of a retired field.  Taking it out moves every field
  // below by 8 bytes, and the v6 kernels' scalar argument loads then merge
  // differently: their object code, compared across cleanups of this header,
  // would change.
  int kernarg_hold_;
  unsigned long long *trace;  // optional: [kTraceSteps][grid][8] s_memrealtime stamps
  int allow_local;  // pinned v6: hand off through the shared L2 when placement allows it
  int xpd;          // generic: XCD slots per direction (0: plain block mapping); v6: 1 when XCD-pinned
  int ring;         // v6: hand-off images reused every `ring` steps (0: one image per step; forward: ring after the T step images)
  int fcopy;        // v6 forward, XCD-pinned: h images also written through (sc1) per step for a streamed projection
  float *xch;       // generic: per-step exchange images [T][dirs][KG][Npad][16] (workspace)
  int poll_sleep;   // v6: s_sleep between flag polls
  int gla;          // v6 forward IO waves: steps ahead the G rows are fetched (3 or 7; 8 LDS slots)
  int e_sc1;        // v6 backward: dGates rows written through (sc1) for a streaming consumer
  int ysc1;         // v6 forward: y rows written through (sc1) and the aggregated epochs published
                    // for the next component's projection streamed off them (launch_chain_rows)
  int bfpart;       // v6 backward, bf16 mode: partial dh exchanged as bf16
  unsigned *cmax;   // v6 backward: column max |DX| [dirs * nW * H] (GRU: then |E|), as float bits
  unsigned *reg;    // v6 backward: per-device registration word (+1 per workgroup at start)
  // v6 backward, bf16 (RnnReserveLayout::pk): dGates written straight into the
  // packed bf16 operands of the GEMMs after the recurrence, instead of fp32
  // rows that pack kernels re-read: dxr = DX rows [dir][T*N][nW*H] (A of the
  // dx GEMM), dxt = DX^T [dir][nW*H][kbt64] (A of dW), et = E^T (A of dR; ==
  // dxt for an LSTM), frames along the packed rows (kbt64 >= T*N, zero tail)
  __bf16 *dxr, *dxt, *et;
  long kbt64;
  // bf16 one-layer bidirectional (bf16_io): the forward writes its output h as
  // packed bf16 too -- yr = rows [T*N][dirs*H] (A of the next component's
  // input projection), yc = columns [dirs*H][kbt64] (B of this component's dR
  // and of the next component's dW) -- and the backward then writes E^T
  // shifted by one step (eshift: direction 0 frame f at f - N, direction 1 at
  // f + N), so that dR pairs it with the unshifted yc
  __bf16 *yr, *yc;
  int eshift;
  // v6 backward, fp32 partials, ring of 2: self-tagged hand-off (see
  // rnn_bwd_rec6): the consumers poll the partial-dh words themselves instead
  // of the producers' epoch flags; taken by the slots probe6 finds XCD-local
  // (v6 forward, split-fp16 without IO waves: the same for the h hi / lo
  // halves, each carrying the tag in its LSB)
  int dtag;
};

// Phase stamps of the first kTraceSteps steps ([steps][grid][16]; thread 0 of every workgroup;
// 100 MHz constant clock), only when the host passes a trace buffer
// (KCTC_REC_TRACE): 0 step start, 1 flags seen, 2 operand loads landed,
// 3 MFMA + K reduction done, 4 published (+ flag), 5 step end.
// v6 backward: slots 16 + w flags seen by wave w, 24 + w its hand-off loads landed.
constexpr int kTraceSteps = 256, kTraceStride = 32;
// (the cursor trc_ / trg_ of REC_TRACE_INIT lives in VGPRs: the stamps cost
// the step loop no scalar registers)
#define REC_TRACE_INIT                                                                    \
  unsigned long long *trc_ = p.trace ? p.trace + (long)blockIdx.x * kTraceStride : nullptr; \
  long trg_ = (long)gridDim.x * kTraceStride;                                             \
  asm volatile("" : "+v"(trc_), "+v"(trg_))
#define REC_TRACE(kk, ph)                                                                 \
  do {                                                                                    \
    if (trc_ && threadIdx.x == 0 && (kk) < kTraceSteps) {                                 \
      unsigned long long *tr_ = trc_ + (long)(kk) * trg_;                                 \
      tr_[(ph)] = __builtin_amdgcn_s_memrealtime();                                       \
      if ((ph) == 2 || (ph) == 3) tr_[12 + (ph)] = __builtin_amdgcn_s_memtime();          \
    }                                                                                     \
  } while (0)
// per-wave stamps (lane 0 of every wave): slot 6 + w loads landed, 10 + w MFMA done;
// slots 14/15: shader-clock counter (s_memtime) at phases 2/3 (clock estimate)
#define REC_TRACE_W(kk, ph)                                                               \
  do {                                                                                    \
    if (trc_ && (threadIdx.x & 63) == 0 && (kk) < kTraceSteps)                            \
      trc_[(long)(kk) * trg_ + (ph) + (threadIdx.x >> 6)] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)

// Hand-off of the generic recurrences (placement-independent): payload sc1
// stores (put) -> every storing wave s_waitcnt vmcnt(0) -> workgroup barrier
// -> ONE lane stores the step epoch (sc1) into the workgroup's flag word
// (signal_epoch); consumers: wave 0 polls the nwg flag words of its direction
// with one sc1 load per lane, barrier (wait_flags), then every wave loads the
// payload with sc1 loads (MI355X_MICROARCH.md "Valid forms", row 1).  Polling
// traffic: 4 B per producer, not the whole payload.
__device__ __forceinline__ void wait_flags(const unsigned *flags, int nwg, unsigned epoch,
                                           unsigned *err, int &bad, int *bad_lds) {
  if (threadIdx.x < 64) {
    int spins = 0;
    while (true) {
      bool ok = true;
      for (int i = threadIdx.x; i < nwg; i += 64)
        ok &= __hip_atomic_load(flags + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= epoch;
      if (__all(ok)) break;
      if (++spins > kSpinLimit ||
          ((spins & 255) == 0 && __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
        bad = 1;
        if (threadIdx.x == 0) *bad_lds = 1;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
  }
  __syncthreads();
  if (*bad_lds) bad = 1;
}

__device__ __forceinline__ floatx4 ld4(const float *p) { return *reinterpret_cast<const floatx4 *>(p); }
__device__ __forceinline__ void st4(float *p, floatx4 v) { *reinterpret_cast<floatx4 *>(p) = v; }

__device__ __forceinline__ unsigned xcc_id() {
  unsigned v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
  return v & 0xfu;
}

__device__ __forceinline__ float fsigm(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
__device__ __forceinline__ float ftanh(float x) { return 2.f * fsigm(2.f * x) - 1.f; }

__device__ __forceinline__ void put(float *q, float v, int local) {
  if (local) {
    __hip_atomic_store(reinterpret_cast<unsigned *>(q), __float_as_uint(v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_WORKGROUP);
  } else {
    __hip_atomic_store(reinterpret_cast<unsigned *>(q), __float_as_uint(v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  }
}

__device__ __forceinline__ void signal_epoch(unsigned *flag, unsigned epoch, int local) {
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // every storing wave drains
  __syncthreads();
  if (threadIdx.x == 0) {
    if (local) __hip_atomic_store(flag, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else __hip_atomic_store(flag, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

constexpr int kMaxEPT = 4;  // (n, unit) elements per thread: N * U <= 1024

typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
// products of the v6 recurrences: split-fp16 (fp32-class) or bf16
enum { kPrecX3 = 0, kPrecBf16 = 1, kPrecX3S = 2 };
// kPrecX3S: split-fp16 with the hi and lo parts stacked in ONE 16-row MFMA
// operand -- for row groups of <= 8 sequences, whose tiles leave rows 8..15
// empty: A = [hi rows 0..7; lo rows 0..7], acc += A B_hi + A B_lo, then row r
// + row r + 8 = hi B_hi + hi B_lo + lo B_hi + lo B_lo (all four terms: 2 MFMAs
// per block instead of 3, and the lo x lo term the 3-MFMA form drops)

// max over each aligned group of U (8, 16, 32) lanes, all lanes active
__device__ __forceinline__ float group_maxU(float v, int U) {
  v = U > 8 ? group_max16(v) : group_max8(v);
  if (U > 16) v = fmaxf(v, __shfl_xor(v, 16));
  return v;
}


// v6 flag words: one 128-B line per (direction, workgroup), so that the
// producers' flag stores and the consumers' polls spread over L2 / memory
// channels instead of hammering one line.
constexpr int kFlagStride = 32;  // words
// Words of the flag area (zeroed before every recurrence launch) with a name.
// Host side, after the component's recurrences are done: the dynamic tile
// counters of the dW / dR weight GEMMs and the item counters of their packs
constexpr int kTileWordW = 1008, kTileWordR = 1009;
constexpr int kPackWord = 1010, kPackWords = 5;  // 1010..1014
// where an XCD-pinned backward recurrence's workgroups OR in 1 << XCC_ID
constexpr int kXcdWord = 1016;
constexpr int kResWord = 1017;  // v6 recurrence: workgroups resident so far (beside_recurrence)
constexpr int kGateWord = 1018;  // blocks of its residency gate that left (rnn_resident_gate)
constexpr int kFlag6Word = 1024;  // the first v6 flag line
constexpr int kAggLine = 256;     // the first aggregated line, counted from kFlag6Word (agg_flag6)
// the named words: apart, the host's counters below the recurrence's words,
// all inside the words below the v6 flag lines
static_assert(kTileWordW < kTileWordR && kTileWordR < kPackWord && kPackWord + kPackWords <= kXcdWord &&
                  kXcdWord < kResWord && kResWord < kGateWord && kGateWord < kFlag6Word,
              "named flag words: distinct, the counters below the recurrence's words, all below the v6 flag lines");
__device__ __forceinline__ unsigned *flag6(const RecParams &p, int grp, int d, int g, int nwg) {
  return p.flags + kFlag6Word + (((long)grp * p.dirs + d) * nwg + g) * kFlagStride;
}
// aggregated epoch of (row group, direction) for the streamed GEMMs of an
// XCD-pinned recurrence: one line each, 256 lines past the flag lines
__device__ __forceinline__ unsigned *agg_flag6(const RecParams &p, int grp, int d) {
  return p.flags + kFlag6Word + (kAggLine + (long)grp * p.dirs + d) * kFlagStride;
}
__device__ __forceinline__ void wait_flags6(const unsigned *f0, int nwg, unsigned epoch, unsigned *err, int &bad,
                                            int *bad_lds, int sleep = 1) {
  if (threadIdx.x < 64) {
    int spins = 0;
    while (true) {
      bool ok = true;
      for (int i = threadIdx.x; i < nwg; i += 64)
        ok &= __hip_atomic_load(f0 + (long)i * kFlagStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= epoch;
      if (__all(ok)) break;
      if (++spins > kSpinLimit ||
          ((spins & 255) == 0 && __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
        bad = 1;
        if (threadIdx.x == 0) {
          *bad_lds = 1;
          if (spins > kSpinLimit) atomicOr(err, 0x10000u);  // this wait ran out of time itself
        }
        break;
      }
      if (sleep) __builtin_amdgcn_s_sleep(1);
    }
  }
  __syncthreads();
  if (*bad_lds) bad = 1;
}
// Per-wave wait (the forward's flagged hand-off): a wave waits only for the
// producers whose rows IT loads -- lane j polls producer prod (-1: none) --
// and goes on to its own loads and MFMAs while the other waves still wait, so
// the hand-off of the last producer to publish costs only the loads of the
// waves that read it.  No workgroup barrier (the step's next one follows the
// K reduction); a timeout sets *bad_lds for the barrier after.
__device__ __forceinline__ bool wave_wait_prod(const unsigned *f0, int prod, unsigned epoch, unsigned *err,
                                               int *bad_lds, int sleep) {
  int spins = 0;
  while (true) {
    const bool ok =
        prod < 0 || __hip_atomic_load(f0 + (long)prod * kFlagStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= epoch;
    if (__all(ok)) return true;
    if (++spins > kSpinLimit ||
        ((spins & 255) == 0 && __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
      if ((threadIdx.x & 63) == 0) *bad_lds = 1;
      return false;
    }
    if (sleep) __builtin_amdgcn_s_sleep(1);
  }
}

// Placement probe of a v6 launch in XCD-slot mapping: 1 iff every workgroup of
// direction d reads the same HW_REG_XCC_ID (then the hand-off may stay in that
// XCD's L2: plain payload and flag stores, sc1 loads).  Publishes epoch 1.
__device__ int probe6(const RecParams &p, int grp, int d, int g, int nwg, int &bad, int *bad_lds, int *loc_lds) {
  unsigned *ids = p.flags + 512 + (grp * p.dirs + d) * nwg;
  const unsigned me = xcc_id() + 1u;
  if (threadIdx.x == 0) __hip_atomic_store(ids + g, me, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  signal_epoch(flag6(p, grp, d, g, nwg), 1u, 0);
  wait_flags6(flag6(p, grp, d, 0, nwg), nwg, 1u, p.err, bad, bad_lds);
  if (threadIdx.x < 64) {
    bool ok = true;
    for (int i = threadIdx.x; i < nwg; i += 64)
      ok &= __hip_atomic_load(ids + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == me;
    const bool all = __all(ok);
    if (threadIdx.x == 0) *loc_lds = all ? 1 : 0;
  }
  __syncthreads();
  return *loc_lds;
}

// 4-byte LDS-DMA (global_load_lds_dword): lane l's dword to LDS byte address
// lds + 4 l.  Inline asm, so that the compiler's wait-count pass does not see
// it: a pending LDS-DMA there merges into the other waves' code paths of
// the same kernel and turns their exact vmcnt waits into vmcnt(0).  The
// issuing wave waits for it with explicit s_waitcnt and reads none of it.
// M0 (a reserved register) is saved and restored inside the statement.
__device__ __forceinline__ void dma_lds_dword(const float *g, unsigned lds) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(g), "s"(lds)
      : "memory");
}

// the same, system-coherent (sc1): data written by another XCD while this
// kernel runs (a concurrent producer's write-through stores)
__device__ __forceinline__ void dma_lds_dword_sc1(const void *g, unsigned lds) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off sc1\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(g), "s"(lds)
      : "memory");
}

// A system-coherent 4-byte load that has landed when the statement ends, and
// a write-through 4-byte store, both invisible to the compiler's wait-count
// pass: memory operations it can see on the IO waves' paths merge into the
// hand-off waves' paths at the barriers and make their exact waits
// conservative (measured: a forward with such polls 2.06 -> 2.4 us/step).
__device__ __forceinline__ unsigned ld_u32_sc1_now(const unsigned *g) {
  unsigned v;
  asm volatile("global_load_dword %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(g) : "memory");
  return v;
}
__device__ __forceinline__ void st_u32_sc1(unsigned *g, unsigned v) {
  asm volatile("global_store_dword %0, %1, off sc1" ::"v"(g), "v"(v) : "memory");
}

// Workgroup barrier for LDS hand-offs.  RAW = true: the LDS writes drained
// and s_barrier, without __syncthreads' fence -- with LDS-DMA in flight the
// fence waits for every outstanding vector memory operation (vmcnt(0)),
// which would turn the IO waves' G fetch three steps ahead into one step and
// hold the hand-off waves on their own stores.  Only for barriers that order
// LDS traffic alone.
template <bool RAW>
__device__ __forceinline__ void lds_barrier() {
  if constexpr (RAW) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  } else {
    __syncthreads();
  }
}

// exponent s with max * 2^s in [2^13, 2^14) (s = 14 for max == 0)
__device__ __forceinline__ int split_exp(float mx) {
  int e = 0;
  (void)frexpf(mx, &e);
  return 14 - e;
}

__device__ __forceinline__ void split16(float x, _Float16 &hi, _Float16 &lo) {
  hi = (_Float16)x;
  lo = (_Float16)(x - (float)hi);
}

// v6 shapes that compile: H in {256, 320, 512, 1024}; U in {8, 16} at 256
// threads, U = 16 (H = 512) or 32 at 512 threads (H / (16 * waves) output tiles
// per wave and H / U producers in groups of 512 / (4 U) for the backward)
template <int U, int H, int NTH>
constexpr bool v6_shape_ok() {
  return (NTH == (U == 32 ? 512 : 256) || (U == 16 && NTH == 512 && H == 512)) && H % (16 * (NTH / 64)) == 0 &&
         (H / U) % (NTH / (4 * U)) == 0;
}
// The instantiation a V6Cfg names.  K::get<MODE, U, H, NTH, P>() returns the
// kernel's address; the recursion only spells the template arguments.
template <class K, int MODE, int U, int H, int NTH, int P>
const void *rec6_of_shape() {
  if constexpr (v6_shape_ok<U, H, NTH>()) return K::template get<MODE, U, H, NTH, P>();
  else throw std::logic_error("v6 recurrence: shape not compiled");
}
template <class K, int MODE, int U, int NTH, int P>
const void *rec6_of_h(int H) {
  switch (H) {
    case 256: return rec6_of_shape<K, MODE, U, 256, NTH, P>();
    case 320: return rec6_of_shape<K, MODE, U, 320, NTH, P>();
    case 512: return rec6_of_shape<K, MODE, U, 512, NTH, P>();
    case 1024: return rec6_of_shape<K, MODE, U, 1024, NTH, P>();
    default: throw std::logic_error("v6 recurrence: H not compiled");
  }
}
template <class K, int MODE, int P>
const void *rec6_of_cfg(int H, const V6Cfg &c) {
  switch (c.U) {
    case 8: return rec6_of_h<K, MODE, 8, 256, P>(H);
    case 16:
      if (c.nth != 512) return rec6_of_h<K, MODE, 16, 256, P>(H);
      if constexpr (P == kPrecX3) {
        if (c.variant == kRec6Stacked) return rec6_of_h<K, MODE, 16, 512, kPrecX3S>(H);
      }
      if (c.variant == kRec6IoWave) return rec6_of_h<K, MODE, 16, 512, P | 4>(H);
      return rec6_of_h<K, MODE, 16, 512, P>(H);
    default: return rec6_of_h<K, MODE, 32, 512, P>(H);
  }
}
template <class K>
const void *rec6_of(int mode, int prec, int H, const V6Cfg &c) {
  if (mode == kLstm) return prec == kPrecBf16 ? rec6_of_cfg<K, kLstm, kPrecBf16>(H, c) : rec6_of_cfg<K, kLstm, kPrecX3>(H, c);
  return prec == kPrecBf16 ? rec6_of_cfg<K, kGru, kPrecBf16>(H, c) : rec6_of_cfg<K, kGru, kPrecX3>(H, c);
}

}  // namespace
}  // namespace kctc
