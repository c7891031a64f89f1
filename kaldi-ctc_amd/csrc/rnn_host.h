// rnn_host.h -- what the units of the RNN host share, private to csrc/ (the
// map of the units is rnn.hip's header).  rnn_plan.h holds what is decided
// once per call (workspace view, recurrence plan); this header declares the
// steps the passes are made of, each defined in exactly one unit, and the
// state that must exist once (events, the exchange pool, the trace flags).
#pragma once
#include <algorithm>

#include "common.h"
#include "elementwise.h"
#include "gemm.h"
#include "gemm_x3p.h"
#include "prof.h"
#include "rec_common.h"
#include "rec_gate.h"
#include "rnn.h"
#include "rnn_plan.h"

namespace kctc {

// ---- rnn.hip: what every pass shares ---------------------------------------
// Stacked layer l in the parameter vector: direction 0's block at pl0 (W
// first), direction 1's pls floats on; within a block R, bW and bR
struct LayerW {
  long pl0, pls, roff, bW, bR;
};
LayerW layer_w(const RnnDesc &d, int l);

// The checks of a call entry, one place each; every entry makes them in its
// own order (and range_ok before the rest, where it checks the range at all)
bool range_ok(const RnnDesc &d, int T, int N);
struct RnnCall {
  const RnnReserveLayout lay;
  const RnnWs ws;
  RecPlan pl;
  const RnnDesc &d; const int N;
  RnnCall(const RnnDesc &dd, int T, int n, void *workspace)
      : lay(rnn_reserve_layout(dd, T, n)), ws(dd, T, n, workspace), d(dd), N(n) {}
  bool reserve_fits(size_t res_bytes) const { return res_bytes >= sizeof(float) * (size_t)lay.total; }
  bool workspace_fits(size_t ws_bytes) const { return ws_bytes >= ws.bytes(); }
  bool plan(bool fwd) { pl = plan_rec(d, N, fwd); return (bool)pl; }  // false: no recurrence runs this shape
};

// KCTC_REC_TRACE=<dir>: trace the first forward and the first backward
// recurrence launch of the process into <dir>/rec_{fwd,bwd}.bin
// (int32 header {grid, steps, nwg, T, dirs, version, xpd, stride} then [steps][grid][stride] uint64 stamps).
struct RecTrace {
  unsigned long long *dev = nullptr;
  size_t n = 0;
  bool arm(const char *tag, int grid);
  void dump(const char *tag, hipStream_t s, int grid, int nwg, int T, int dirs, int ver, int xpd = 1);
};
// RecParams has no linkage (rec_common.h: every unit, host or kernel, compiles
// its own copy), so the steps that take one and that two units need are
// inline here; they own no state.  The streamed launches see the launched
// recurrence through RecLive instead: the fields of RecParams they use, under
// the same names and copied by live() below -- kept in step with RecParams by
// hand; a field a streamed launch starts to read is added in both places.
struct RecLive {
  unsigned *flags;
  int xpd, nwg, dirs, rg, gs;
  const float *xch, *y, *DX;
};
namespace {
inline RecLive live(const RecParams &p) { return {p.flags, p.xpd, p.nwg, p.dirs, p.rg, p.gs, p.xch, p.y, p.DX}; }

// A recurrence kernel (rec6_kernel / rec_generic_kernel) on `nth` threads per workgroup; it was compiled
// against its own translation unit's copy of RecParams: the layouts agree only through rec_common.h
inline void launch_rec(const void *k, const RecParams &p, dim3 grid, int nth, size_t lds, hipStream_t s) {
  (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  void *args[] = {const_cast<RecParams *>(&p)};
  KCTC_HIP_CHECK(hipLaunchKernel(k, grid, dim3(nth), args, lds, s));
}

// What a forward and a backward recurrence of stacked layer l have in common;
// enqueues the reset of the flag area on s.
inline RecParams rec_params(const RnnDesc &d, const RecPlan &pl, const RnnWs &ws, int T, int N, const float *wl,
                            const LayerW &lw, float *R0, const RnnReserveLayout &lay, float *y, unsigned *err,
                            hipStream_t s) {
  RecParams p{};
  p.T = T; p.N = N; p.H = d.H; p.dirs = d.dirs; p.U = pl.U; p.nwg = pl.nwg;
  p.Npad = (N + 15) / 16 * 16;
  p.w = wl; p.pl_stride = lw.pls; p.r_off = lw.roff; p.bR_off = lw.bR;
  p.G = R0 + lay.G; p.y = y; p.aux = R0 + lay.aux; p.err = err;
  p.flags = ws.flags();
  KCTC_HIP_CHECK(hipMemsetAsync(p.flags, 0, kFlagBytes, s));
  p.xpd = pl.xpd;
  p.rg = pl.rg;
  p.gs = pl.gs;
  // XCD-pinned v6 (RecPlan::xcds): each (row group, direction) on one XCD, the
  // hand-off in that XCD's L2 through a ring of two step images
  p.ring = pl.ver == 6 && p.xpd ? 2 : 0;
  return p;
}

// The planned recurrence on s (traced when KCTC_REC_TRACE asks for it); from
// here to the end of the host call the side launches go beside it (v6)
inline void launch_planned(const RnnDesc &d, const RecPlan &pl, bool fwd, RecParams &p, RecTrace &tr,
                           RecScope &scope, hipStream_t s) {
  if (tr.arm(fwd ? "fwd" : "bwd", pl.grid)) p.trace = tr.dev;
  const void *k = pl.ver == 6 ? rec6_kernel(fwd, d.mode, d.prec, d.H, pl.c6)
                              : rec_generic_kernel(fwd, d.mode, p.Npad / 16);
  {
    ProfSpan ps(s, fwd ? "rnn_fwd_rec" : "rnn_bwd_rec");
    launch_rec(k, p, dim3(pl.grid), pl.nth, pl.lds, s);
  }
  KCTC_HIP_CHECK(hipGetLastError());
  if (pl.ver == 6) scope.enqueued(p.flags, p.dirs * p.nwg * p.rg);
  else scope.none();
}
}  // namespace

// The v6 backward's exchange pool (library-owned, one per device)
float *xch_acquire(size_t bytes, hipStream_t s);
void xch_release(hipStream_t s);
// An event recorded on s now (one per thread), and s waiting for what `other` holds now
hipEvent_t fork_event(hipStream_t s);
void join_stream(hipStream_t s, hipStream_t other);
// `side` from here on beside the recurrence just launched: after the event
// recorded before it (null: side waited for it already), once it is resident
void go_beside(hipStream_t side, hipEvent_t fork);
extern thread_local bool g_last_bwd_scratch_free;  // rnn_last_bwd_scratch_free

// The XCDs pinned recurrences ran on and the XCDs in use: PackAvoid without a
// counter, X3PArgs::avoid_word / avoid_xcds
PackAvoid avoid_pair();
// k blocks of a contraction over K in precision bf (bf16: 64 wide) or split-fp16 (32)
inline int kblocks(bool bf, long K) { return (int)(bf ? (K + 63) / 64 : (K + 31) / 32); }
// Rows / columns of X packed for the precision: bf16 (no exponents), or
// split-fp16 with exponents into e -- rows from `bound` or the row maximum,
// columns from `bound` (> 0) or the column maxima computed here into cm
void pack_rows(bool bf, hipStream_t s, const float *X, long ldx, int R, int K, _Float16 *out, int *e, float bound,
               int batch = 1, long sX = 0, long sOut = 0, long sE = 0);
void pack_cols(bool bf, hipStream_t s, const float *X, long ldx, int R, int Cn, int shift, _Float16 *out, int *e,
               unsigned *cm, float bound, PackAvoid av = {});
// output^T of every direction shifted by one step (h_prev of the dR product:
// direction 0 pairs frame t with y(t - 1), direction 1 with y(t + 1)) on s:
// [dirs][H][KB][64] into Yt; split-fp16 exponents eY [dirs][H] from the
// column maxima cm [dirs][H] or (null) the bound 1; av: counters counter + dir
void pack_shifted_y(bool bf, hipStream_t s, const float *out, int dirs, int H, long TN, int N, _Float16 *Yt, int *eY,
                    const unsigned *cm, PackAvoid av = {});
// C (M x N, ldc) = A B^T on operands packed for the precision: what the bf16
// and split-fp16 arms share (bf16 drops the exponents)
X3PArgs packed_product(bool bf, int M, int N, int KB, const _Float16 *A, const int *eA, const _Float16 *B,
                       const int *eB, float *C, long ldc);
// W rows of a projection (both directions, [dirs][G][KB][64], exponents
// [dirs][G]) packed on s, and the product G = in W^T + bW (+ bR) but for its
// A operand
X3PArgs proj_product(const RnnDesc &d, const RnnWs &ws, hipStream_t s, long TN, int l, const float *wl, int KB,
                     float *G);
// W^T of layer l's dx GEMM on s: [dirs][Din][KB][64] into Bp, exponents eB
// [dirs][Din]; the column maxima of direction dir at cm + dir * cm_dir (0: one reused)
void pack_dx_wt(const RnnDesc &d, hipStream_t s, int l, const float *wl, int KB, _Float16 *Bp, int *eB, unsigned *cm,
                long cm_dir);

// ---- rnn_stream.hip: what may stream, and the streamed launches ----------------
bool bwd_dx_stream_ok(const RecPlan &pl, const RnnDesc &d, int l, int T, int N);
bool chain_ok(const RecPlan &pl, const RnnDesc &d, int T, int N, const RnnFwdChain *c);
bool chain_rows_ok(const RecPlan &pl, const RnnDesc &d, int T, int N, const RnnFwdChain *c);
void launch_chain_proj(const RnnDesc &d, const RecLive &p, hipEvent_t fork, int T, int N, RnnFwdChain &c,
                       unsigned *err);
void launch_chain_rows(const RnnDesc &d, const RecLive &p, hipEvent_t fork, int T, int N, RnnFwdChain &c,
                       unsigned *err);
void pack_dx_weights(const RnnDesc &d, int l, const float *w, const RnnWs &ws, hipStream_t st);
void launch_bwd_stream(const RnnDesc &d, const RecLive &p, int l, const float *w, float *dxl, const RnnWs &ws,
                       int T, int N, hipStream_t ov, hipEvent_t fork, unsigned *err, const RnnPrepack *pre);
bool wgrad_stream_ok(const RecPlan &pl, const RnnDesc &d, int T, int N);
bool wgrad_stream_shape(const RnnDesc &d, int T, int N);
void launch_wgrad_stream(const RecPlan &pl, const RnnDesc &d, const RecLive &p, hipEvent_t fork, int T, int N,
                         const float *y, const RnnWs &ws, void *reserve, unsigned *err, RnnWgradStream &wgrad,
                         hipStream_t s);

// ---- rnn_fwd.hip: where the length-aware training passes keep their images ----
// Byte offsets.  Workspace: [rnn_workspace_bytes | g: G before the shift, then
// the backward's E before the shift back | g2: a GRU's DX likewise | dy: one
// layer's aligned dy].  Reserve: [rnn_reserve_layout | xz: the input with its
// padding zeroed (the weight GEMMs read it) | ysh: every stacked layer's
// output in the shifted frame, ysh_layer apart (the backward recurrence reads
// h and c there)].  Unidirectional: G is projected in place, but the dGates
// still pass through g / g2: a v6 hand-off that tags its payload words leaves
// denormals where the padding steps' gradients are zero in exact arithmetic,
// and the pass back writes those rows as +0.
struct SeqTrainLay {
  size_t ws0, g, g2, dy, ws_total;
  size_t res0, xz, ysh, ysh_layer, res_total;
  SeqTrainLay(const RnnDesc &d, int T, int N);
};
// The checks the three length-aware training entries share (KRNN_OK: lens is set)
struct SeqLens;
int seq_train_entry(const RnnDesc &d, int T, int N, const int *seq_lengths, size_t ws_bytes, size_t res_bytes,
                    SeqLens *lens);

// ---- rnn_wgrad.hip: what the weight-gradient stream launches per chunk --------
void wgrad_frames(const RnnDesc &d, hipStream_t s, int T, int N, const float *x, const float *y, const RnnWs &ws,
                  float *dw, void *reserve, int max_blocks, float in_bound, int dir, int ta, int tb);
void wgrad_bias(const RecPlan &pl, const RnnDesc &d, hipStream_t s, int T, int N, float *dw, void *reserve, int l);

}  // namespace kctc
