// rnn_plan.h -- what the RNN host (the units mapped in rnn.hip) decides once
// per call, private to csrc/: the workspace view (RnnWs) and the recurrence
// plan (RecPlan) of rnn_plan.hip.  Both are built per host call and never kept
// across calls: the environment knobs and the CU budget may change in between.
// (rnn_host.h, beside this header, declares the steps those units share.)
#pragma once
#include <algorithm>
#include <cstdlib>

#include "rec_common.h"
#include "rnn.h"

namespace kctc {

inline int env_int(const char *name, int dflt) {
  const char *v = getenv(name);
  return v ? atoi(v) : dflt;
}
// The RNN GEMMs run on the packed split-fp16 matrix-core path (x3p_gemm.hip, gemm_x3p.h)
// unless the contraction is too short to pay for packing.
inline bool use_x3(int K, int min_k = 128) { return K >= min_k; }
// |x| <= 1: an LSTM / GRU / TANH layer output
inline bool bounded_out(const RnnDesc &d) { return d.mode != kRelu; }
// bf16 recurrences write their dGates straight into the packed bf16 GEMM
// operands (RecParams::dxr / dxt / et) -- v6 only (a v6 backward runs for
// every bf16 shape), whole 64-element gate rows
// (one-layer descriptors -- the recipe's components; a stacked descriptor's
// weight gradients measured wrong with it, so those keep the pack path)
inline bool bf16_direct(const RnnDesc &d, int ver) {
  return d.prec == kPrecBf16 && ver == 6 && (d.nw() * d.H) % 64 == 0 && d.layers == 1 && d.pk;
}
// ... and, one-layer bidirectional, the forward writes its output packed
// (RecParams::yr / yc) and the backward E^T shifted (eshift); H % 32 == 0 so
// that a workgroup's units fill whole 16-B row chunks
inline bool bf16_io(const RnnDesc &d) {
  return bf16_direct(d, 6) && d.layers == 1 && d.dirs == 2 && d.H % 32 == 0 && (2 * d.H) % 64 == 0 && d.pkio;
}

// CUs of one XCD (generic: one direction's workgroups per XCD slot; v6: a
// pinned (row group, direction) on one XCD)
constexpr int kCusPerXcd = 32;
// flag region: words 0..1023 (generic flags, placement ids, the named words of
// rec_common.h), then one 128-B line per (direction, workgroup) for v6
constexpr size_t kFlagBytes = 4096 + 512 * 128;  // v6: up to 4 row groups x 2 dirs x 64 workgroups

// Packed split-fp16 GEMM operands of one layer at a time (forward,
// backward-data and the weight GEMMs of a component never overlap):
//   forward   : input rows [TN][Din], W rows [dirs*G][Din]
//   bwd data  : dGates rows [dirs*TN][G], W^T rows [dirs*Din][G]
//   bwd weight: dGates^T [dirs*G][TN] (+ GRU: E^T), input^T [Din][TN],
//               shifted output^T [dirs*H][TN]
// plus int exponents and float-bit column maxima (G = nW*H).  Byte offsets
// from the pack area's start.
struct PackLay {
  size_t a, b, c, ea, eb, ec, ed, cm, part, cnt, part2, cme, fcnt, fpart, wt, ewt, cmw, xt, yt, ext, eyt, pcnt, total;
};

// The workspace of (d, T, N): the split-K slabs of the weight-gradient GEMMs,
// the recurrence flag words, the generic exchange images (v6 forward: its
// step images), then the pack area.  Built once per host call.
struct RnnWs {
  PackLay lay;
  long split_floats = 0;  // floats of the split slabs (dR's, then dW's)
  size_t flags_off = 0, xch_off = 0, pack_off = 0;
  char *base = nullptr;
  RnnWs(const RnnDesc &d, int T, int N, void *workspace);
  size_t bytes() const { return pack_off + lay.total; }  // rnn_workspace_bytes
  template <typename P>
  P *at(size_t off) const { return reinterpret_cast<P *>(base + pack_off + off); }  // off: a PackLay field
  unsigned *flags() const { return reinterpret_cast<unsigned *>(base + flags_off); }
  float *xch() const { return reinterpret_cast<float *>(base + xch_off); }
  float *split_slab() const { return reinterpret_cast<float *>(base); }
};

// Which recurrence (d, N) runs in one direction of time, and how it is
// launched.  ver 0: not supported (bf16 exists on v6 only; no U fits).
struct RecPlan {
  int ver = 0;   // 6: v6; 4: the generic kernels (rec_generic.hip)
  int U = 0;     // units per workgroup
  V6Cfg c6;      // ver == 6
  int nth = 0, nwg = 0;  // threads per workgroup, workgroups per (row group, direction)
  size_t lds = 0;        // dynamic LDS bytes
  int rg = 1, gs = 16;   // v6 row groups (RecParams::rg / gs)
  int xpd = 0;           // RecParams::xpd: generic XCD slots per direction (0: plain mapping); v6 1 when XCD-pinned
  unsigned xcds = 0;     // XCDs a pinned v6 recurrence occupies (bit x: XCD x), else 0
  int wgs = 0;           // dirs * nwg * rg
  unsigned grid = 0;
  bool scratch_free = false;  // v6: the kernel runs without scratch (else nothing runs beside it)
  explicit operator bool() const { return ver != 0; }
};
RecPlan plan_rec(const RnnDesc &d, int N, bool fwd);

// persistent blocks a streamed GEMM may run beside a recurrence of `rec_wgs`
// workgroups (rnn.h, CU budget); 0: too few to stream
int stream_block_budget(int rec_wgs, bool backward);

}  // namespace kctc
