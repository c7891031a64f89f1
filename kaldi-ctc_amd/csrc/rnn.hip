// rnn.hip -- cuDNN-v5 compatible LSTM / GRU / RELU / TANH layers for gfx950.
//
// Replaces cudnnRNNForwardTraining / BackwardData / BackwardWeights as the
// reference calls them (src/cudamatrix/cudnn-recurrent.cc:13-102 through
// src/nnet2/nnet-cudnn-component.cc:508-614).  Per stacked layer:
//
// Forward
//   1. G = x W^T + bW (+ bR): the input projection of all T*N frames of both
//      directions as one packed split-fp16 GEMM (x3p_gemm.hip) -- or, for the
//      layers above the first, streamed off the previous component's running
//      recurrence (launch_chain_proj / launch_chain_rows).
//   2. rnn_fwd_rec6: ONE persistent launch runs the whole time recurrence of
//      both directions (and of every row group of 8 or 16 sequences).  Work-
//      group (group, dir, g) owns hidden units [g*U, g*U+U); its slice of R
//      (nW*U gate rows x H) is held for the whole launch in REGISTERS as
//      split-fp16 MFMA B fragments (bf16 in configs[4]'s precision).  Per step
//      it loads h_{t-1} of its direction as fp16 hi/lo A fragments (sc1
//      buffer loads of the step's exchange image), multiplies on
//      v_mfma_f32_16x16x32_f16 (K split over the waves, reduced through LDS in
//      a fixed order), applies the gates (cell state in registers) and
//      publishes its U units of h_t as hi/lo fp16 with sc1 16-B stores.
// Backward data
//   rnn_bwd_rec6, reduce-scatter form: per step a workgroup sums the partial
//   dh of its own units from the direction's H/U producers (fixed order), adds
//   dy, does the pointwise cell backward (dc in registers), multiplies its
//   dGates by its R rows (registers) and publishes the partial dh of ALL H
//   units (MFMA C-fragment layout).  dGates rows go to the reserve, from where
//   the dx GEMM of the layer below is streamed while the recurrence runs
//   (x3p_bwd_stream_kernel).
// Backward weights
//   dW += dGx^T x, dR += dGh^T h_prev (time-shifted views), packed split-fp16
//   GEMMs on a side stream beside the next component's backward recurrence;
//   bias sums accumulated by the recurrence.
// Hand-off protocols of the v6 recurrences (the kernel files have the detail):
//   flagged: payload sc1 stores -> every storing wave's s_waitcnt vmcnt(0) ->
//     workgroup barrier -> lane 0 stores the step epoch into the workgroup's
//     own 128-B flag line; consumers poll the flag lines of their producers,
//     then sc1 loads (MI355X_MICROARCH.md "Valid forms", row 1).  The bf16
//     recurrences, the unpinned ones, the IO-wave forward and a pinned forward
//     that copies its images for a streamed projection hand off this way.
//   self-tagged (RecParams::dtag): the XCD-pinned split-fp16 recurrences hand
//     off through a ring of two step images in their XCD's L2 whose words
//     carry the step's tag themselves; the consumers poll the payload, no
//     flag store and no drain before it.  The epoch lines are still written
//     for the streamed GEMMs outside the XCD (epoch_lines).
// Every spin is bounded (3 s); a timeout sets the device error word, every
// workgroup drains out and the train step fails loudly.
// One generic kernel pair (fp32 MFMA, all-gather of h / dGates per step through
// epoch flags, XCD-slot block mapping where the shape has whole slots) runs
// the shapes v6 does not compile (RELU / TANH, other H).  This file is the
// host side of the three entry points; which recurrence runs and where the
// workspace's parts lie: rnn_plan.hip (plan_rec, RnnWs); what may run beside
// a recurrence: rec_gate.hip; the kernels: rec6_fwd.hip, rec6_bwd.hip,
// rec_generic.hip, rec_common.h.
//
// Semantics follow cuDNN v5 as used by CuDNNRecurrentComponent: hx = cx = 0,
// dhy = dcy = 0 (SetBufferZero, nnet-cudnn-component.cc:494-506), all N
// sequences run the full T steps (no masking), weights in the opaque layout of
// nnet-cudnn-component.cc:327-413 (see RnnDesc::lin_offset).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

#include "common.h"
#include "elementwise.h"
#include "gemm.h"
#include "gemm_x3p.h"
#include "prof.h"
#include "rec_common.h"
#include "rec_gate.h"
#include "rnn.h"
#include "rnn_plan.h"
#include "seq_align.h"

namespace kctc {

long RnnDesc::params_size() const {
  long t = 0;
  for (int l = 0; l < layers; l++) t += dirs * pl_size(l);
  return t;
}

long RnnDesc::lin_offset(int p, int lin, bool bias) const {
  long off = 0;
  for (int q = 0; q < p; q++) off += pl_size(q / dirs);
  const int layer = p / dirs, di = din(layer);
  const long n = nw();
  if (!bias) {
    if (lin < n) return off + (long)lin * H * di;
    return off + n * H * (long)di + (long)(lin - n) * H * H;
  }
  return off + n * H * (long)di + n * H * (long)H + (long)lin * H;
}

void rnn_set_precision(RnnDesc &d, int prec) {
  d.prec = prec;
  const char *e = getenv("KCTC_BF16_DIRECT");
  d.pk = !e || atoi(e) != 0;
  e = getenv("KCTC_BF16_IO");
  d.pkio = !e || atoi(e) != 0;
}

namespace {

// Stacked layer l in the parameter vector: direction 0's block at pl0 (W
// first), direction 1's pls floats on; within a block R, bW and bR
struct LayerW {
  long pl0, pls, roff, bW, bR;
};
LayerW layer_w(const RnnDesc &d, int l) {
  LayerW lw;
  lw.pl0 = d.lin_offset(l * d.dirs, 0, false);
  lw.pls = d.pl_size(l);
  lw.roff = d.lin_offset(l * d.dirs, d.nw(), false) - lw.pl0;
  lw.bW = d.lin_offset(l * d.dirs, 0, true) - lw.pl0;
  lw.bR = d.lin_offset(l * d.dirs, d.nw(), true) - lw.pl0;
  return lw;
}

// A recurrence kernel (rec6_kernel / rec_generic_kernel) on `nth` threads per workgroup; it was compiled
// against its own translation unit's copy of RecParams: the layouts agree only through rec_common.h
void launch_rec(const void *k, const RecParams &p, dim3 grid, int nth, size_t lds, hipStream_t s) {
  (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  void *args[] = {const_cast<RecParams *>(&p)};
  KCTC_HIP_CHECK(hipLaunchKernel(k, grid, dim3(nth), args, lds, s));
}

// KCTC_REC_TRACE=<dir>: trace the first forward and the first backward
// recurrence launch of the process into <dir>/rec_{fwd,bwd}.bin
// (int32 header {grid, steps, nwg, T, dirs, version, xpd, stride} then [steps][grid][stride] uint64 stamps).
struct RecTrace {
  unsigned long long *dev = nullptr;
  size_t n = 0;
  bool arm(const char *tag, int grid) {
    static bool done_fwd = false, done_bwd = false;
    const char *dir = getenv("KCTC_REC_TRACE");
    if (!dir || !*dir) return false;
    bool &done = tag[0] == 'f' ? done_fwd : done_bwd;
    if (done) return false;
    done = true;
    n = (size_t)kTraceSteps * grid * kTraceStride;
    KCTC_HIP_CHECK(hipMalloc(&dev, n * sizeof(unsigned long long)));
    KCTC_HIP_CHECK(hipMemset(dev, 0, n * sizeof(unsigned long long)));
    return true;
  }
  void dump(const char *tag, hipStream_t s, int grid, int nwg, int T, int dirs, int ver, int xpd = 1) {
    if (!dev) return;
    KCTC_HIP_CHECK(hipStreamSynchronize(s));
    std::vector<unsigned long long> h(n);
    KCTC_HIP_CHECK(hipMemcpy(h.data(), dev, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    (void)hipFree(dev);
    dev = nullptr;
    std::string path = std::string(getenv("KCTC_REC_TRACE")) + "/rec_" + tag + ".bin";
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return;
    int hdr[8] = {grid, kTraceSteps, nwg, T, dirs, ver, xpd, kTraceStride};
    fwrite(hdr, sizeof(int), 8, f);
    fwrite(h.data(), sizeof(unsigned long long), n, f);
    fclose(f);
  }
};

// What a forward and a backward recurrence of stacked layer l have in common;
// enqueues the reset of the flag area on s.
RecParams rec_params(const RnnDesc &d, const RecPlan &pl, const RnnWs &ws, int T, int N, const float *wl,
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
void launch_planned(const RnnDesc &d, const RecPlan &pl, bool fwd, RecParams &p, RecTrace &tr, RecScope &scope,
                    hipStream_t s) {
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

// Per-device exchange pool of the v6 backward: one step image per time step,
// never reused within a launch (T x dirs x nwg x H x Npad floats, 4.2 GB for
// BLSTM-512 N=16 T=2000).  Library-owned so that the components of a network
// share it; launches on one device are ordered through its event.
struct XchPool {
  void *p = nullptr;
  size_t bytes = 0;
  hipEvent_t ev = nullptr;
};
std::mutex g_xch_mu;
XchPool g_xch[64];

float *xch_acquire(size_t bytes, hipStream_t s) {
  int dev = 0;
  KCTC_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_xch_mu);
  XchPool &x = g_xch[dev & 63];
  if (x.ev) KCTC_HIP_CHECK(hipStreamWaitEvent(s, x.ev, 0));
  if (bytes > x.bytes) {
    if (x.p) {
      KCTC_HIP_CHECK(hipDeviceSynchronize());
      KCTC_HIP_CHECK(hipFree(x.p));
      x.p = nullptr;
    }
    KCTC_HIP_CHECK(hipMalloc(&x.p, bytes));
    x.bytes = bytes;
  }
  return static_cast<float *>(x.p);
}
void xch_release(hipStream_t s) {
  int dev = 0;
  KCTC_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_xch_mu);
  XchPool &x = g_xch[dev & 63];
  if (!x.ev) KCTC_HIP_CHECK(hipEventCreateWithFlags(&x.ev, hipEventDisableTiming));
  KCTC_HIP_CHECK(hipEventRecord(x.ev, s));
}

// The recurrence and a GEMM streaming off it must run at the same time, so
// the GEMM's stream forks from the recurrence's stream at an event recorded
// BEFORE the recurrence launch, and the GEMM is enqueued AFTER it: should the
// two streams share a hardware queue, the GEMM then merely runs after the
// recurrence instead of blocking it (its blocks only wait for recurrence flags).
hipEvent_t fork_event(hipStream_t s) {
  static thread_local hipEvent_t ev = nullptr;
  if (!ev) KCTC_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  KCTC_HIP_CHECK(hipEventRecord(ev, s));
  return ev;
}
void join_stream(hipStream_t s, hipStream_t other) {
  static thread_local hipEvent_t ev = nullptr;
  if (!ev) KCTC_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  KCTC_HIP_CHECK(hipEventRecord(ev, other));
  KCTC_HIP_CHECK(hipStreamWaitEvent(s, ev, 0));
}

// ---------------------------------------------------------------------------
// GEMMs streamed off a running v6 recurrence
// ---------------------------------------------------------------------------
// The epoch lines a stream consumer polls for the launched recurrence `p`:
// its workgroups' flag lines (flag6), or, XCD-pinned -- the flags then stay
// in the XCD's L2 -- the sc1 copies of its epochs (agg_flag6)
const unsigned *epoch_lines(const RecParams &p) {
  return p.flags + kFlag6Word + (p.xpd ? kAggLine * kFlagStride : 0);
}

// XCDs whose every CU an XCD-pinned recurrence holds: a streamed GEMM's
// blocks landing there leave at once (xcd_word / xcd_count), and the launch
// has 8 / (8 - pinned) times the blocks so that its budget stays.  0 when the
// recurrence is not pinned or its slots take half an XCD each (configs[2]:
// all eight XCDs, 16 of each XCD's CUs left to the stream: there its blocks
// stay, on the CUs the recurrence leaves).
int whole_pinned_xcds(const RecParams &p) {
  const int n = p.xpd && p.nwg == kCusPerXcd ? p.dirs * p.rg : 0;
  return n < 8 ? n : 0;
}

// The producer side of a streamed launch beside the recurrence `p`, for a
// budget of `budget` persistent blocks
struct StreamProducer {
  const unsigned *lines;  // epoch_lines
  int nwg;                // lines per (row group, direction): one when pinned (aggregated)
  const unsigned *xcd_word = nullptr;  // pinned: where the recurrence's XCDs register,
  int xcd_count = 0;                   // and how many of them
  int blocks;             // the budget, scaled so that it stays beside the blocks that leave the pinned XCDs
};
StreamProducer stream_producer(const RecParams &p, int budget) {
  StreamProducer sp;
  sp.lines = epoch_lines(p);
  sp.nwg = p.xpd ? 1 : p.nwg;
  const int pinned = whole_pinned_xcds(p);
  if (pinned) { sp.xcd_word = p.flags + kXcdWord; sp.xcd_count = pinned; }
  sp.blocks = pinned ? budget * 8 / (8 - pinned) : budget;
  return sp;
}

// Is the dx of layer l streamed off its v6 backward recurrence `pl`
// (launch_bwd_stream, given a dx buffer and an overlap stream)?  The
// forward's W^T prepack (RnnPrepack) asks the same question.
bool bwd_dx_stream_ok(const RecPlan &pl, const RnnDesc &d, int l, int T, int N) {
  if (pl.ver != 6 || d.dirs != 2 || !env_int("KCTC_BWD_STREAM", 1) || !pl.scratch_free) return false;
  // split-fp16 at N <= 16 by default (KCTC_STREAM_ALL: bf16 and N > 16 too)
  if (!((d.prec == kPrecX3 && N <= 16) || env_int("KCTC_STREAM_ALL", 0))) return false;
  const int G4 = d.nw() * d.H;
  if (!use_x3(G4) || G4 > 4096 || (d.prec != kPrecX3 && G4 % 64)) return false;
  if ((long)T * N * d.din(l) * 4 >= (1L << 31)) return false;
  return stream_block_budget(pl.wgs, true) > 0;
}

bool chain_buffers_ok(const RnnFwdChain *c, int T, int N) {
  return c->ws_bytes >= rnn_workspace_bytes(*c->d, T, N) &&
         c->res_bytes >= sizeof(float) * (size_t)rnn_reserve_layout(*c->d, T, N).total;
}

// Can `c` consume the exchange images of this component's last forward
// recurrence `pl` (v6, bidirectional) as its layer-0 projection input?
bool chain_ok(const RecPlan &pl, const RnnDesc &d, int T, int N, const RnnFwdChain *c) {
  if (!c || !c->d || !c->side || pl.ver != 6 || d.dirs != 2 || !env_int("KCTC_FWD_STREAM", 1)) return false;
  if (!pl.scratch_free) return false;
  const RnnDesc &n = *c->d;
  // split-fp16 into split-fp16, or bf16 images into a bf16 projection
  if (n.D != d.dirs * d.H || !use_x3(n.D) || N > 64 || d.prec != n.prec) return false;
  // default: split-fp16 at N <= 16 only.  Row groups and bf16 run (and are
  // tested) under KCTC_STREAM_ALL=1, but are slower on the recipe shapes: at
  // N = 64 / T = 667 (configs[2]) and bf16 N = 32 (configs[4]) the GEMM on
  // the CUs left beside the 128-workgroup recurrence outlasts it (990k ->
  // 728k and 560k -> 389k frames/s measured), the 256-tile GEMM after it wins
  if ((N > 16 || d.prec == kPrecBf16) && !env_int("KCTC_STREAM_ALL", 0)) return false;
  // an XCD-pinned producer runs faster alone: beside the streamed projection
  // (HBM traffic on the other XCDs) its steps took 0.17-0.3 us longer, more
  // than the 256-tile GEMM after it costs (configs[1]: 555.9k vs 564.8k
  // frames/s same box); KCTC_FWD_STREAM_PINNED=1 streams anyway
  if (pl.xcds && !env_int("KCTC_FWD_STREAM_PINNED", 0)) return false;
  // and only the IO-wave variant carries the copies (not bf16 in 8-row groups: never run pinned with them)
  if (pl.xcds && (pl.c6.variant != kRec6IoWave || (d.prec == kPrecBf16 && pl.gs <= 8))) return false;
  if (!stream_block_budget(pl.wgs, false)) return false;
  const long xs = 2L * (d.H / 32) * (d.prec == kPrecBf16 ? 1 : 2) * 16 * 32 * pl.rg;  // halves per step image
  if ((long)T * xs * 2 >= (1L << 31)) return false;
  return chain_buffers_ok(c, T, N);
}

// Layer-0 projection of the consumer, streamed off the producer's exchange images.
void launch_chain_proj(const RnnDesc &d, const RecParams &p, hipEvent_t fork, int T, int N, RnnFwdChain &c,
                       unsigned *err) {
  KCTC_HIP_CHECK(hipStreamWaitEvent(c.side, fork, 0));  // after the producer's flag reset
  beside_recurrence(c.side);
  const RnnDesc &n = *c.d;
  const bool bf = n.prec == kPrecBf16;
  const int NW = n.nw(), G = NW * n.H, Din = n.D, KB = Din / (bf ? 64 : 32);
  const long pl0 = n.lin_offset(0, 0, false), pls = n.pl_size(0);
  const float *wl = c.w + pl0;
  const RnnWs ws(n, T, N, c.workspace);
  _Float16 *Bp = ws.at<_Float16>(ws.lay.b);
  int *eB = bf ? nullptr : ws.at<int>(ws.lay.eb);
  {
    ProfSpan ps(c.side, "x3_pack_chain");
    if (bf)
      bf16_pack_rows(c.side, wl, Din, G, Din, reinterpret_cast<__bf16 *>(Bp), n.dirs, pls, (long)G * KB * 64);
    else
      x3p_pack_rows(c.side, wl, Din, G, Din, Bp, eB, 0.f, n.dirs, pls, (long)G * KB * 64, (long)G);
  }
  const RnnReserveLayout lay = rnn_reserve_layout(n, T, N);
  X3PArgs x;
  x.bf16 = bf;
  x.M = T * N; x.N = G; x.KB = KB;
  x.A = reinterpret_cast<const _Float16 *>(p.xch); x.eA0 = bf ? 0 : 14;  // x3 images hold h 2^14
  x.B = Bp; x.eB = eB;
  x.C = static_cast<float *>(c.reserve) + lay.G; x.ldc = (long)n.dirs * G;
  x.bias = wl + (n.lin_offset(0, 0, true) - pl0);
  x.bias2 = n.mode == kGru ? nullptr : wl + (n.lin_offset(0, NW, true) - pl0);
  x.batch = n.dirs; x.sB = (long)G * KB * 64; x.seB = bf ? 0 : G; x.sC = G; x.sBias = pls;
  x.tile_counter = reinterpret_cast<int *>(ws.flags());
  // every producer workgroup needs a CU of its own (96 KB LDS); the GEMM's
  // persistent blocks (96 KB each) take the rest minus a margin (chain_ok
  // checked that at least 8 fit).  No gradient exchange runs during a
  // forward pass: the updates of the previous step waited for it.
  // XCD-pinned producer: the sc1 copies of its epochs, no block on its XCDs
  const StreamProducer sp = stream_producer(p, stream_block_budget(d.dirs * p.nwg * p.rg, false));
  x.stream_flags = sp.lines; x.stream_nwg = sp.nwg; x.stream_T = T; x.stream_N = N;
  x.stream_xcd_word = sp.xcd_word; x.stream_xcd_count = sp.xcd_count;
  x.max_blocks = sp.blocks;
  x.stream_group_step = 2L * (d.H / 32) * (bf ? 1 : 2) * 16 * 32;  // rnn_fwd_rec6's XG
  x.stream_rg = p.rg; x.stream_gs = p.gs; x.stream_step = x.stream_group_step * p.rg; x.stream_err = err;
  // K split by producer direction: the work is ready from the first steps
  // (KCTC_STREAM_DIRSPLIT=0: whole-K tiles from the middle of the sequence outwards)
  if (env_int("KCTC_STREAM_DIRSPLIT", 1)) {
    x.stream_arrive = ws.at<int>(ws.lay.fcnt);
    x.stream_part = ws.at<float>(ws.lay.fpart);
  }
  {
    ProfSpan ps(c.side, "fwd_proj_stream");
    gemm_x3p(c.side, x);
  }
  c.done = true;
}

// Can `c`'s layer-0 projection stream off this component's y rows
// (launch_chain_rows)?  Split-fp16 into split-fp16, the 256-tile row stream.
bool chain_rows_ok(const RecPlan &pl, const RnnDesc &d, int T, int N, const RnnFwdChain *c) {
  if (!c || !c->d || !c->side || pl.ver != 6 || d.dirs != 2 || d.prec == kPrecBf16 ||
      !env_int("KCTC_FWD_STREAM", 1))
    return false;
  if (!pl.scratch_free) return false;
  const RnnDesc &n = *c->d;
  const long TN = (long)T * N;
  if (n.D != d.dirs * d.H || n.prec != d.prec || !use_x3(n.D) || d.H % 32 || d.H > 4096 || T < 2) return false;
  if (!x3p_bwd_stream_256((int)TN, n.dirs * n.nw() * n.H, d.H / 32, false)) return false;
  if (TN * n.dirs * n.nw() * n.H * 4 >= (1L << 31) || TN * (d.H / 32) * 128 >= (1L << 31)) return false;
  // at N <= 16 (configs[1]); larger batches run the 256-tile GEMM after the
  // recurrence (shorter recurrences, less time to hide the GEMM behind)
  if (N > 16 && !env_int("KCTC_STREAM_ALL", 0)) return false;
  if (!stream_block_budget(pl.wgs, false)) return false;
  return chain_buffers_ok(c, T, N);
}

// The consumer's layer-0 projection G' = [y_fwd | y_bwd] W'^T + b' streamed
// off this forward recurrence's y rows (written through, p.ysc1): the
// direction-split row stream of gemm_x3p_bwd_stream with a forward producer --
// the K half of direction 0 of frame t is out at producer step t, direction
// 1's at step T - 1 - t, so each 256 x 256 tile of G' is two half-K jobs whose
// partials meet (plus the biases) in the second.  The K halves of W' are
// packed as rows of their own (per-half exponents).
void launch_chain_rows(const RnnDesc &d, const RecParams &p, hipEvent_t fork, int T, int N, RnnFwdChain &c,
                       unsigned *err) {
  KCTC_HIP_CHECK(hipStreamWaitEvent(c.side, fork, 0));  // after the producer's flag reset
  // not before every workgroup of the recurrence is resident: dispatched
  // first (another queue), 32 blocks per XCD would take every CU of an XCD
  // the recurrence is pinned to before its first workgroup got there (seen
  // once as a 3-s stream-wait timeout, error 0x2)
  beside_recurrence(c.side);
  const RnnDesc &n = *c.d;
  const int NW = n.nw(), G = NW * n.H, H = d.H, KBh = H / 32, Din = n.D;
  const long TN = (long)T * N;
  const long pl0 = n.lin_offset(0, 0, false), pls = n.pl_size(0);
  const float *wl = c.w + pl0;
  const RnnWs ws(n, T, N, c.workspace);
  _Float16 *Bp = ws.at<_Float16>(ws.lay.b);
  int *eB = ws.at<int>(ws.lay.eb);
  const long sB = (long)n.dirs * G * KBh * 64;
  {
    ProfSpan ps(c.side, "x3_pack_chain");
    for (int h = 0; h < 2; h++)  // K half h of the rows of both consumer directions
      x3p_pack_rows(c.side, wl + h * H, Din, G, H, Bp + h * sB, eB + h * n.dirs * G, 0.f, n.dirs, pls,
                    (long)G * KBh * 64, G);
  }
  const RnnReserveLayout lay = rnn_reserve_layout(n, T, N);
  X3PBwdStream a;
  a.forward = true;
  a.M = (int)TN; a.N = n.dirs * G; a.KB = KBh;
  a.E = p.y; a.lde = 2L * H; a.edoff = H;
  a.Ap = ws.at<_Float16>(ws.lay.a); a.eA = ws.at<int>(ws.lay.ea);
  a.B = Bp; a.eB = eB; a.sB = sB; a.seB = n.dirs * G;
  a.C = static_cast<float *>(c.reserve) + lay.G; a.ldc = (long)n.dirs * G;
  a.bias = wl + (n.lin_offset(0, 0, true) - pl0);
  a.bias2 = n.mode == kGru ? nullptr : wl + (n.lin_offset(0, NW, true) - pl0);
  a.bias_cols = G; a.sbias = pls;
  a.part = ws.at<float>(ws.lay.fpart);
  a.part2 = ws.at<float>(ws.lay.part2);
  a.cnt = ws.at<int>(ws.lay.cnt);
  // 128: every CU the recurrence leaves (configs[1]: 96 -> 128 blocks 720k -> 751k frames/s)
  const StreamProducer sp =
      stream_producer(p, std::min(128, stream_block_budget(d.dirs * p.nwg * p.rg, false)));
  a.flags = sp.lines; a.nwg = sp.nwg; a.T = T; a.Nf = N; a.err = err; a.rg = p.rg;
  a.xcd_word = sp.xcd_word; a.xcd_count = sp.xcd_count;
  a.blocks = sp.blocks;
  {
    ProfSpan ps(c.side, "fwd_proj_rows");
    gemm_x3p_bwd_stream(c.side, a);
  }
  c.done = true;
}

// W^T of layer l's dx GEMM (B operand of the streamed GEMM) into the
// workspace slot wt (per-column exponents ewt, absmax scratch cmw)
void pack_dx_weights(const RnnDesc &d, int l, const float *w, const RnnWs &ws, hipStream_t st) {
  const bool bf = d.prec == kPrecBf16;
  const int G4 = d.nw() * d.H, KB = G4 / (bf ? 64 : 32), Din = d.din(l);
  const long pl0 = d.lin_offset(l * d.dirs, 0, false), pls = d.pl_size(l);
  const float *wl = w + pl0;
  _Float16 *Bp = ws.at<_Float16>(ws.lay.wt);
  int *eB = ws.at<int>(ws.lay.ewt);
  unsigned *cm = ws.at<unsigned>(ws.lay.cmw);
  ProfSpan ps(st, "x3_pack_bwd_stream");
  for (int dir = 0; dir < 2; dir++) {
    if (bf) {
      bf16_pack_cols(st, wl + dir * pls, Din, G4, Din, 0, reinterpret_cast<__bf16 *>(Bp) + (long)dir * Din * KB * 64);
      continue;
    }
    absmax_f32(st, wl + dir * pls, Din, G4, Din, nullptr, cm + dir * Din);
    x3p_pack_cols(st, wl + dir * pls, Din, G4, Din, 0, Bp + (long)dir * Din * KB * 64, eB + dir * Din, cm + dir * Din,
                  0.f);
  }
}

// dx of stacked layer l on `ov`, streamed off the backward recurrence `p`
// just launched (gemm_x3p_bwd_stream): W_d^T packed first (unless the forward
// did), then one persistent launch that packs dGates rows as the recurrence
// flags them.
void launch_bwd_stream(const RnnDesc &d, const RecParams &p, int l, const float *w, float *dxl, const RnnWs &ws,
                       int T, int N, hipStream_t ov, hipEvent_t fork, unsigned *err, const RnnPrepack *pre) {
  KCTC_HIP_CHECK(hipStreamWaitEvent(ov, fork, 0));  // after the flag reset, not after the recurrence
  // not before every workgroup of the recurrence is resident: its blocks
  // wait (on_pinned_xcd) for the pinned recurrence's XCDs to register, and a
  // block parked on one of those XCDs' CUs before the recurrence's last
  // workgroup got there would keep it out (with W^T packed by the forward
  // the GEMM starts together with the recurrence)
  beside_recurrence(ov);
  const bool bf = d.prec == kPrecBf16;
  const int G4 = d.nw() * d.H, KB = G4 / (bf ? 64 : 32), Din = d.din(l);
  const long TN = (long)T * N;
  // packed by the forward on its side stream (RnnPrepack), else here
  if (pre && pre->done) KCTC_HIP_CHECK(hipStreamWaitEvent(ov, pre->ev, 0));
  else pack_dx_weights(d, l, w, ws, ov);
  X3PBwdStream a;
  a.bf16 = bf;
  a.M = (int)TN; a.N = Din; a.KB = KB;
  a.E = p.DX; a.lde = 2L * G4; a.edoff = G4;
  a.Ap = ws.at<_Float16>(ws.lay.a); a.eA = ws.at<int>(ws.lay.ea);
  a.B = ws.at<_Float16>(ws.lay.wt); a.eB = bf ? nullptr : ws.at<int>(ws.lay.ewt);
  a.sB = (long)Din * KB * 64; a.seB = Din;
  a.C = dxl; a.ldc = Din;
  a.part = ws.at<float>(ws.lay.part);
  a.part2 = ws.at<float>(ws.lay.part2);
  a.cnt = ws.at<int>(ws.lay.cnt);
  // 128 measured best at configs[1] since the self-tagged recurrences (96
  // before: 655.7k -> 670.7k frames/s); never more than the CU budget leaves
  // beside the recurrence and the exchange's kernels (rnn.h).  Blocks landing
  // on the pinned XCDs exit at once: launch enough that ~128 stay
  // 256-tile launch: 48 blocks keep up with the recurrence and leave the
  // other CUs beside it to the weight GEMMs (rnn_backward_weights beside)
  const bool t256 = x3p_bwd_stream_256(a.M, a.N, a.KB, bf);
  // XCD-pinned recurrence: its epochs' sc1 copies (the L2 flags are not
  // visible here), and no block on the recurrence's XCDs
  const StreamProducer sp =
      stream_producer(p, std::min(t256 ? 64 : 128, stream_block_budget(d.dirs * p.nwg * p.rg, true)));
  a.flags = sp.lines; a.nwg = sp.nwg; a.T = T; a.Nf = N; a.err = err; a.rg = p.rg;
  a.xcd_word = sp.xcd_word; a.xcd_count = sp.xcd_count;
  a.blocks = sp.blocks;
  ProfSpan ps(ov, "bwd_data_stream");
  gemm_x3p_bwd_stream(ov, a);
}

// ---------------------------------------------------------------------------
// host: forward training
// ---------------------------------------------------------------------------
// G = in W^T + bW (+ bR) of one stacked layer, both directions, on s: packed
// bf16, packed split-fp16, or (a contraction too short to pack) fp32
void project_input(const RnnDesc &d, const RnnWs &ws, hipStream_t s, long TN, int l, const float *in,
                   const void *in_rows, const float *wl, const LayerW &lw, float *G) {
  const int NW = d.nw(), H = d.H, dirs = d.dirs, Din = d.din(l);
  const long ldc = (long)dirs * NW * H;
  const float *bias = wl + lw.bW, *bias2 = (d.mode == kGru) ? nullptr : wl + lw.bR;
  if (d.prec == kPrecBf16 && use_x3(Din, 32)) {
    // bf16 gate GEMM: input rows and W rows packed as bf16, fp32 accumulation
    // the input rows come packed from the previous component's forward (in_rows)
    const bool rows_in = l == 0 && in_rows && Din % 64 == 0;
    __bf16 *Ap = rows_in ? static_cast<__bf16 *>(const_cast<void *>(in_rows)) : ws.at<__bf16>(ws.lay.a);
    __bf16 *Bp = ws.at<__bf16>(ws.lay.b);
    const int KB = (Din + 63) / 64;
    {
      ProfSpan ps(s, "x3_pack");
      if (!rows_in) bf16_pack_rows(s, in, Din, (int)TN, Din, Ap);
      bf16_pack_rows(s, wl, Din, NW * H, Din, Bp, dirs, lw.pls, (long)NW * H * KB * 64);
    }
    X3PArgs x;
    x.bf16 = true;
    x.M = (int)TN; x.N = NW * H; x.KB = KB;
    x.A = reinterpret_cast<const _Float16 *>(Ap); x.B = reinterpret_cast<const _Float16 *>(Bp);
    x.C = G; x.ldc = ldc; x.bias = bias; x.bias2 = bias2;
    x.batch = dirs; x.sA = 0; x.sB = (long)NW * H * KB * 64;
    x.sC = (long)NW * H; x.sBias = lw.pls;
    ProfSpan ps(s, "gemm_fwd_proj");
    gemm_x3p(s, x);
  } else if (use_x3(Din, 32)) {
    // input rows (a lower stacked layer's output is bounded; the component
    // input and RELU outputs get per-row exponents) and W rows, packed
    _Float16 *Ap = ws.at<_Float16>(ws.lay.a), *Bp = ws.at<_Float16>(ws.lay.b);
    int *eA = ws.at<int>(ws.lay.ea), *eB = ws.at<int>(ws.lay.eb);
    const int KB = (Din + 31) / 32;
    {
      ProfSpan ps(s, "x3_pack");
      x3p_pack_rows(s, in, Din, (int)TN, Din, Ap, eA, (l > 0 && bounded_out(d)) ? 1.f : 0.f);
      x3p_pack_rows(s, wl, Din, NW * H, Din, Bp, eB, 0.f, dirs, lw.pls, (long)NW * H * KB * 64, (long)NW * H);
    }
    X3PArgs x;
    x.M = (int)TN; x.N = NW * H; x.KB = KB;
    x.A = Ap; x.B = Bp; x.eA = eA; x.eB = eB;
    x.C = G; x.ldc = ldc; x.bias = bias; x.bias2 = bias2;
    x.batch = dirs; x.sA = 0; x.seA = 0; x.sB = (long)NW * H * KB * 64; x.seB = (long)NW * H;
    x.sC = (long)NW * H; x.sBias = lw.pls;
    ProfSpan ps(s, "gemm_fwd_proj");
    gemm_x3p(s, x);
  } else {
    GemmArgs g;
    g.transA = false; g.transB = true;
    g.M = (int)TN; g.N = NW * H; g.K = Din;
    g.A = in; g.lda = Din;
    g.B = wl; g.ldb = Din;
    g.C = G; g.ldc = ldc;
    g.bias = bias; g.bias2 = bias2;
    g.batch = dirs; g.strideA = 0; g.strideB = lw.pls; g.strideC = (long)NW * H; g.strideBias = lw.pls;
    ProfSpan ps(s, "gemm_fwd_proj");
    gemm_f32(s, g);
  }
}

// The forward's share of RecParams, and the fills its hand-off needs, on s
void fwd_rec_params(RecParams &p, const RnnDesc &d, const RecPlan &pl, const RnnWs &ws, float *R0,
                    const RnnReserveLayout &lay, bool chained, bool rowchain, hipStream_t s) {
  const long TN = (long)p.T * p.N;
  p.ncol = (d.nw() * pl.U + 15) / 16 * 16;
  p.allow_local = 0;
  p.xch = ws.xch();
  p.poll_sleep = 1;
  p.gla = 3;  // G rows fetched 3 steps ahead (IO waves)
  if (pl.ver != 6) return;
  if (bf16_io(d)) {  // the output also as packed bf16 rows and columns
    p.yr = reinterpret_cast<__bf16 *>(R0 + lay.pkyr);
    p.yc = reinterpret_cast<__bf16 *>(R0 + lay.pkyc);
    p.kbt64 = lay.kbt64;
    if (lay.kbt64 > TN)
      KCTC_HIP_CHECK(hipMemset2DAsync(p.yc + TN, sizeof(__bf16) * lay.kbt64, 0, sizeof(__bf16) * (lay.kbt64 - TN),
                                      (size_t)d.dirs * d.H, s));
  }
  // XCD-pinned: a streamed projection gets sc1 copies of the step images and flags
  p.fcopy = p.xpd && chained;
  p.ysc1 = rowchain ? 1 : 0;
  p.allow_local = p.xpd ? 1 : 0;
  // self-tagged hand-off (the kernel takes it for split-fp16 variants other
  // than kRec6IoWave, without a write-through copy): the ring starts at tag 1
  p.dtag = d.prec != kPrecBf16 && p.ring == 2 && !p.fcopy && p.T >= 2;
  if (p.dtag) {  // rnn_fwd_rec6's ring: after T step images of XS = 64 H rg halves (2 dirs, hi / lo, 16 rows)
    const size_t xs = sizeof(_Float16) * 64 * (size_t)d.H * p.rg;
    KCTC_HIP_CHECK(hipMemsetAsync(reinterpret_cast<char *>(p.xch) + xs * p.T, 0x01, 2 * xs, s));
  }
}

// x^T of the weight GEMMs beside the forward recurrence, off its XCDs
// (rnn_backward_weights' packs; RnnPrepack::wgrad)
void prepack_x_cols(const RnnDesc &d, const RnnWs &ws, const float *in, long TN, const RnnPrepack &pre) {
  hipStream_t ss = pre.stream;
  const int Din = d.din(0);
  int *pc = ws.at<int>(ws.lay.pcnt);  // item counters
  KCTC_HIP_CHECK(hipMemsetAsync(pc, 0, sizeof(int) * 3, ss));
  const unsigned *av = rnn_pinned_xcds();
  const int nx = std::max(1, rnn_usable_cus() / kCusPerXcd);
  ProfSpan ps(ss, "x3_pack_w_fwd");
  x3p_pack_cols(ss, in, Din, (int)TN, Din, 0, ws.at<_Float16>(ws.lay.xt), ws.at<int>(ws.lay.ext), nullptr,
                pre.in_bound, 1, 0, 0, 0, 0, av, nx, pc);
}
// ... and y^T after it (and after the joins: s does not wait for it)
void prepack_y_cols(const RnnDesc &d, const RnnWs &ws, const float *out, long TN, int N, RnnPrepack &pre,
                    hipStream_t s) {
  hipStream_t ss = pre.stream;
  KCTC_HIP_CHECK(hipStreamWaitEvent(ss, fork_event(s), 0));
  const int H = d.H, dirs = d.dirs;
  const long KBt = (TN + 31) / 32;
  int *pc = ws.at<int>(ws.lay.pcnt);
  const unsigned *av = rnn_pinned_xcds();
  const int nx = std::max(1, rnn_usable_cus() / kCusPerXcd);
  const long ldy = (long)dirs * H;
  {
    ProfSpan ps(ss, "x3_pack_w_fwd");
    for (int dir = 0; dir < dirs; dir++)
      x3p_pack_cols(ss, out + (long)dir * H, ldy, (int)TN, H, dir == 0 ? N : -N,
                    ws.at<_Float16>(ws.lay.yt) + (long)dir * H * KBt * 64, ws.at<int>(ws.lay.eyt) + dir * H,
                    nullptr, 1.f, 1, 0, 0, 0, 0, av, nx, pc + 1 + dir);
  }
  KCTC_HIP_CHECK(hipEventRecord(pre.wev, ss));
  pre.wdone = true;
}

}  // namespace

thread_local bool g_last_bwd_scratch_free = true;
bool rnn_last_bwd_scratch_free() { return g_last_bwd_scratch_free; }

bool rnn_packed_output(const RnnDesc &d, int T, int N, void *reserve, const void **rows, const void **cols) {
  *rows = *cols = nullptr;
  if (!bf16_io(d) || !reserve) return false;
  const RnnReserveLayout lay = rnn_reserve_layout(d, T, N);
  float *res = static_cast<float *>(reserve);
  *rows = res + lay.pkyr;
  *cols = res + lay.pkyc;
  return true;
}

int rnn_forward_training(const RnnDesc &d, hipStream_t s, int T, int N, const float *x,
                         const float *w, float *y, void *workspace, size_t ws_bytes,
                         void *reserve, size_t res_bytes, unsigned *err, RnnFwdChain *chain,
                         bool input_projected, const void *in_rows, RnnPrepack *pre) {
  RecScope rec_scope;  // the side launches' residency gates (beside_recurrence)
  if (chain) chain->done = false;
  if (pre) pre->done = pre->wdone = false;
  if (T <= 0 || N <= 0 || N > 16 * kMaxRT || d.H % 16) return KRNN_NOT_SUPPORTED;
  const RnnReserveLayout lay = rnn_reserve_layout(d, T, N);
  if (res_bytes < sizeof(float) * (size_t)lay.total) return KRNN_BAD_PARAM;
  const RnnWs ws(d, T, N, workspace);
  if (ws_bytes < ws.bytes()) return KRNN_BAD_PARAM;
  const RecPlan pl = plan_rec(d, N, true);
  if (!pl) return KRNN_NOT_SUPPORTED;
  const bool v6 = pl.ver == 6;
  const int dirs = d.dirs;
  const long TN = (long)T * N;
  float *res = static_cast<float *>(reserve);
  const float *in = x;
  for (int l = 0; l < d.layers; l++) {
    const bool last = l == d.layers - 1;
    float *R0 = res + lay.per_layer * l;
    float *out = last ? y : R0 + lay.out;
    const LayerW lw = layer_w(d, l);
    const float *wl = w + lw.pl0;
    // (layer 0 may come projected: streamed by the previous component)
    if (!(l == 0 && input_projected)) project_input(d, ws, s, TN, l, in, in_rows, wl, lw, R0 + lay.G);
    RecParams p = rec_params(d, pl, ws, T, N, wl, lw, R0, lay, out, err, s);
    // what runs beside this recurrence: the next component's projection off
    // its step images or its y rows, and (one-layer descriptors) the packs
    // the backward would otherwise wait for -- W^T of its streamed dx GEMM
    // (rnn_backward_data's `streamed` shapes), x^T / y^T of its weight GEMMs
    const bool chained = last && chain_ok(pl, d, T, N, chain);
    const bool rowchain = !chained && last && chain_rows_ok(pl, d, T, N, chain);
    fwd_rec_params(p, d, pl, ws, R0, lay, chained, rowchain, s);
    const bool prepack = pre && pre->dx && pre->stream && pre->ev && v6 && d.layers == 1 &&
                         bwd_dx_stream_ok(plan_rec(d, N, false), d, 0, T, N);
    const bool prepack_w = pre && pre->stream && pre->wev && pre->wgrad && pre->in_bound > 0.f && v6 &&
                           d.layers == 1 && d.prec != kPrecBf16 && T > 1 && bounded_out(d) && use_x3((int)TN) &&
                           pl.scratch_free;
    const hipEvent_t fork = (chained || prepack || prepack_w || rowchain) ? fork_event(s) : nullptr;
    RecTrace tr;
    launch_planned(d, pl, true, p, tr, rec_scope, s);
    if (prepack) {  // beside the recurrence, once it is resident
      KCTC_HIP_CHECK(hipStreamWaitEvent(pre->stream, fork, 0));
      beside_recurrence(pre->stream);
      pack_dx_weights(d, 0, w, ws, pre->stream);
      KCTC_HIP_CHECK(hipEventRecord(pre->ev, pre->stream));
      pre->done = true;
    }
    if (prepack_w) {
      if (!prepack) KCTC_HIP_CHECK(hipStreamWaitEvent(pre->stream, fork, 0));
      beside_recurrence(pre->stream);
      prepack_x_cols(d, ws, in, TN, *pre);
    }
    if (chained) {
      launch_chain_proj(d, p, fork, T, N, *chain, err);
      join_stream(s, chain->side);
    }
    if (rowchain) {
      launch_chain_rows(d, p, fork, T, N, *chain, err);
      join_stream(s, chain->side);
    }
    if (prepack_w) prepack_y_cols(d, ws, out, TN, N, *pre, s);
    tr.dump("fwd", s, pl.grid, p.nwg, T, dirs, pl.ver, p.xpd);
    in = out;
  }
  return KRNN_OK;
}

// ---------------------------------------------------------------------------
// host: length-aware inference (rnn.h rnn_forward_inference_seq)
// ---------------------------------------------------------------------------
namespace {
// the seq buffer: the layer-0 input with its padding zeroed, one layer's
// projected G before the shift, one layer's output before the shift back
struct SeqBuf {
  size_t xz = 0, g = 0, y = 0, total = 0;
  SeqBuf(const RnnDesc &d, int T, int N) {
    const size_t TN = (size_t)T * N;
    xz = 0;
    g = align_up(sizeof(float) * TN * d.D, 256);
    y = g + (d.dirs == 2 ? align_up(sizeof(float) * TN * d.dirs * d.nw() * d.H, 256) : 0);
    total = y + align_up(sizeof(float) * TN * d.dirs * d.H, 256);
  }
};
}  // namespace

size_t rnn_seq_buffer_bytes(const RnnDesc &d, int T, int N) { return SeqBuf(d, T, N).total; }

int rnn_forward_inference_seq(const RnnDesc &d, hipStream_t s, int T, int N, const int *seq_lengths, const float *x,
                              const float *w, float *y, void *workspace, size_t ws_bytes, void *reserve,
                              size_t res_bytes, void *seq_buffer, size_t seq_bytes, unsigned *err) {
  RecScope rec_scope;
  if (T <= 0 || N <= 0 || N > 16 * kMaxRT || d.H % 16) return KRNN_NOT_SUPPORTED;
  SeqLens lens;
  if (!seq_lens(seq_lengths, T, N, &lens)) return KRNN_BAD_PARAM;
  const RnnReserveLayout lay = rnn_reserve_layout(d, T, N);
  if (res_bytes < sizeof(float) * (size_t)lay.total) return KRNN_BAD_PARAM;
  const RnnWs ws(d, T, N, workspace);
  if (ws_bytes < ws.bytes()) return KRNN_BAD_PARAM;
  const SeqBuf sb(d, T, N);
  if (!seq_buffer || seq_bytes < sb.total) return KRNN_BAD_PARAM;
  const RecPlan pl = plan_rec(d, N, true);
  if (!pl) return KRNN_NOT_SUPPORTED;
  const int H = d.H, dirs = d.dirs, NW = d.nw();
  const long TN = (long)T * N;
  char *sbase = static_cast<char *>(seq_buffer);
  float *xz = reinterpret_cast<float *>(sbase + sb.xz), *gs = reinterpret_cast<float *>(sbase + sb.g),
        *ys = reinterpret_cast<float *>(sbase + sb.y);
  float *res = static_cast<float *>(reserve);
  // padding rows of the input may hold anything: zeroed before the projection
  seq_align(s, x, xz, T, N, d.D, d.D, lens);
  const float *in = xz;
  for (int l = 0; l < d.layers; l++) {
    const bool last = l == d.layers - 1;
    float *R0 = res + lay.per_layer * l;
    float *out = last ? y : R0 + lay.out;
    const LayerW lw = layer_w(d, l);
    const float *wl = w + lw.pl0;
    // no streamed hand-over and no packed input rows here: they read
    // un-shifted images
    if (dirs == 2) {
      // the reverse direction's gate columns move right by T - len[n] frames,
      // so that every sequence ends at row T-1 where that recurrence starts
      project_input(d, ws, s, TN, l, in, nullptr, wl, lw, gs);
      seq_align(s, gs, R0 + lay.G, T, N, dirs * NW * H, NW * H, lens);
    } else {
      project_input(d, ws, s, TN, l, in, nullptr, wl, lw, R0 + lay.G);
    }
    RecParams p = rec_params(d, pl, ws, T, N, wl, lw, R0, lay, ys, err, s);
    fwd_rec_params(p, d, pl, ws, R0, lay, false, false, s);
    RecTrace tr;
    launch_planned(d, pl, true, p, tr, rec_scope, s);
    tr.dump("fwd", s, pl.grid, p.nwg, T, dirs, pl.ver, p.xpd);
    // ... and its output moves back; padding rows of both directions become 0
    seq_unalign(s, ys, out, T, N, dirs * H, H, lens);
    in = out;
  }
  return KRNN_OK;
}

// ---------------------------------------------------------------------------
// streamed weight gradients of the bottom component (rnn.h RnnWgradStream)
// ---------------------------------------------------------------------------
namespace {
// the dynamic tile counter of a weight GEMM (flag word kTileWordW / kTileWordR
// of the workspace: the recurrences of this layer, which use the flag area,
// are done); none without a persistent grid
int *tile_counter(const RnnWs &ws, int word, int max_blocks) {
  return max_blocks > 0 ? reinterpret_cast<int *>(ws.flags() + word) : nullptr;
}

// dW_dir += DX_dir^T x and dR_dir += DX_dir^T h_prev over the frames [ta, tb)
// of direction dir (layer 0 of a one-layer component, split-fp16, LSTM: E == DX)
void wgrad_frames(const RnnDesc &d, hipStream_t s, int T, int N, const float *x, const float *y, const RnnWs &ws,
                  float *dw, void *reserve, int max_blocks, float in_bound, int dir, int ta, int tb) {
  if (tb <= ta) return;
  const RnnReserveLayout lay = rnn_reserve_layout(d, T, N);
  const int NW = d.nw(), H = d.H, dirs = d.dirs, G4 = NW * H, Din = d.din(0);
  const long ldg = (long)dirs * G4, ldy = (long)dirs * H;
  const int R = (tb - ta) * N, KB = (R + 31) / 32;
  const float *DX = static_cast<const float *>(reserve) + lay.E;
  _Float16 *DXt = ws.at<_Float16>(ws.lay.a), *Xt = ws.at<_Float16>(ws.lay.b), *Yt = ws.at<_Float16>(ws.lay.c);
  int *eDX = ws.at<int>(ws.lay.ea), *eX = ws.at<int>(ws.lay.eb), *eY = ws.at<int>(ws.lay.ec);
  unsigned *cm = ws.at<unsigned>(ws.lay.cm);
  {
    ProfSpan ps(s, "x3_pack_w");
    const float *src = DX + (long)ta * N * ldg + (long)dir * G4;
    absmax_f32(s, src, ldg, R, G4, nullptr, cm);
    x3p_pack_cols(s, src, ldg, R, G4, 0, DXt, eDX, cm, 0.f);
    const float *xs = x + (long)ta * N * Din;
    if (!(in_bound > 0.f)) absmax_f32(s, xs, Din, R, Din, nullptr, cm + G4);
    x3p_pack_cols(s, xs, Din, R, Din, 0, Xt, eX, cm + G4, in_bound > 0.f ? in_bound : 0.f);
    // h_prev: direction 0 pairs frame t with y(t - 1), direction 1 with y(t + 1);
    // frames outside the sequence contribute zero (pack_cols zero-fills k - shift outside [0, R))
    const float *yd = y + (long)dir * H;
    if (dir == 0) {
      if (ta == 0) x3p_pack_cols(s, yd, ldy, R, H, N, Yt, eY, nullptr, 1.f);
      else x3p_pack_cols(s, yd + (long)(ta - 1) * N * ldy, ldy, R, H, 0, Yt, eY, nullptr, 1.f);
    } else {
      if (tb == T) x3p_pack_cols(s, yd + (long)ta * N * ldy, ldy, R, H, -N, Yt, eY, nullptr, 1.f);
      else x3p_pack_cols(s, yd + (long)(ta + 1) * N * ldy, ldy, R, H, 0, Yt, eY, nullptr, 1.f);
    }
  }
  auto gemm = [&](int n, const _Float16 *B, const int *eB, float *C, int word, const char *name) {
    X3PArgs a;
    a.M = G4; a.N = n; a.KB = KB;
    a.A = DXt; a.eA = eDX; a.B = B; a.eB = eB;
    a.C = C; a.ldc = n; a.beta = 1.f; a.batch = 1;
    a.split_k = x3p_pick_split(G4, n, KB, 1);
    while (a.split_k > 1 && (long)a.split_k * G4 * n > ws.split_floats) a.split_k--;
    a.ws = ws.split_slab();
    a.max_blocks = max_blocks;
    a.tile_counter = tile_counter(ws, word, max_blocks);
    ProfSpan ps(s, name);
    gemm_x3p(s, a);
  };
  gemm(Din, Xt, eX, dw + d.lin_offset(dir, 0, false), kTileWordW, "gemm_bwd_w");
  gemm(H, Yt, eY, dw + d.lin_offset(dir, NW, false), kTileWordR, "gemm_bwd_r");
}

// dbW += sum dGx, dbR += sum dGh of layer l from the partials of its backward recurrence `pl`
void wgrad_bias(const RecPlan &pl, const RnnDesc &d, hipStream_t s, int T, int N, float *dw, void *reserve, int l) {
  const RnnReserveLayout lay = rnn_reserve_layout(d, T, N);
  const int dirs = d.dirs, G4 = d.nw() * d.H;
  const float *R0 = static_cast<const float *>(reserve) + lay.per_layer * l;
  const LayerW lw = layer_w(d, l);
  float *dwl = dw + lw.pl0;
  // (v6: one partial per row group, [group][dir][2][G], added in group order)
  const int rg = pl.ver == 6 ? pl.rg : 1;
  for (int gi = 0; gi < rg; gi++)
    for (int dir = 0; dir < dirs; dir++) {
      const float *part = R0 + lay.bias + ((long)gi * dirs + dir) * 2 * G4;
      clip_sgd_update(s, dwl + dir * lw.pls + lw.bW, part, G4, 1.f, 0.f);
      clip_sgd_update(s, dwl + dir * lw.pls + lw.bR, part + G4, G4, 1.f, 0.f);
    }
}

bool wgrad_stream_ok(const RecPlan &pl, const RnnDesc &d, int T, int N) {
  if (pl.ver != 6 || !use_x3((int)((long)T * N)) || !use_x3(d.nw() * d.H) || !pl.scratch_free) return false;
  return (long)T * N * d.din(0) * 4 < (1L << 31);
}
// Off by default (KCTC_WGRAD_STREAM=1 turns it on): measured on configs[1]
// 470.4k -> 467.0k (2 chunks), 466.1k (4), 454.5k (8) frames/s: the chunk
// GEMMs beside the backward recurrence slow it (33.0 -> 33.3-33.5 ms/step)
// and the per-chunk transposes add packing, more than the 1 ms tail saved.
bool wgrad_stream_shape(const RnnDesc &d, int T, int N) {
  return env_int("KCTC_WGRAD_STREAM", 0) && d.layers == 1 && d.dirs == 2 && d.mode == kLstm && d.prec == kPrecX3 &&
         T >= 8 && N <= 16;
}

// The weight gradients of the bottom component on wgrad.side, chunk by chunk
// as the unpinned backward recurrence `p` just launched on s finishes frames
void launch_wgrad_stream(const RecPlan &pl, const RnnDesc &d, const RecParams &p, hipEvent_t fork, int T, int N,
                         const float *y, const RnnWs &ws, void *reserve, unsigned *err, RnnWgradStream &wgrad,
                         hipStream_t s) {
  // chunk c of C: direction 0 frames [T - b(c+1), T - b(c)), direction 1
  // [b(c), b(c+1)), b(c) = c T / C; complete once every flag line holds
  // epoch b(c+1) + 2 (rows of step k are out at epoch k + 3)
  hipStream_t ws2 = wgrad.side;
  KCTC_HIP_CHECK(hipStreamWaitEvent(ws2, fork, 0));  // after the flag reset
  beside_recurrence(ws2);
  const int C = std::max(1, std::min(wgrad.chunks, T / 4));
  const unsigned *lines = epoch_lines(p);  // (not pinned: the workgroups' own lines)
  const int nlines = p.rg * p.dirs * p.nwg;
  for (int c = 0; c < C; c++) {
    const int b0 = (int)((long)c * T / C), b1 = (int)((long)(c + 1) * T / C);
    rec_epoch_gate(ws2, lines, nlines, (unsigned)(b1 + 2), err);
    wgrad_frames(d, ws2, T, N, wgrad.x, y, ws, wgrad.dw, reserve, wgrad.max_blocks, wgrad.in_bound, 0, T - b1,
                 T - b0);
    wgrad_frames(d, ws2, T, N, wgrad.x, y, ws, wgrad.dw, reserve, wgrad.max_blocks, wgrad.in_bound, 1, b0, b1);
  }
  join_stream(ws2, s);  // the bias partials are written after the last flag
  wgrad_bias(pl, d, ws2, T, N, wgrad.dw, reserve, 0);
  wgrad.done = true;
}
}  // namespace

bool rnn_wgrad_stream_ok(const RnnDesc &d, int T, int N) {
  return wgrad_stream_shape(d, T, N) && wgrad_stream_ok(plan_rec(d, N, false), d, T, N);
}

// ---------------------------------------------------------------------------
// host: backward data (dGates into the reserve, dx)
// ---------------------------------------------------------------------------
namespace {
// The backward's share of RecParams, and the fills its outputs need, on s
void bwd_rec_params(RecParams &p, const RnnDesc &d, const RecPlan &pl, const RnnWs &ws, float *R0,
                    const RnnReserveLayout &lay, const float *dy, float *E, float *DX, bool e_sc1, hipStream_t s) {
  const int NW = d.nw(), H = d.H, dirs = d.dirs, T = p.T, N = p.N;
  const long TN = (long)T * N;
  p.ncol = 16;
  p.dy = dy; p.E = E; p.DX = DX; p.bias = R0 + lay.bias;
  p.allow_local = 0;
  if (pl.ver != 6) {
    p.xch = ws.xch();
    return;
  }
  // XCD-pinned: the partial-dh hand-off in the XCD's L2 (configs[1]: 3.36 ->
  // 2.70 us per step with the streamed dx GEMM beside it (2.41 without),
  // 468k -> 511k frames/s)
  p.allow_local = 1;
  p.poll_sleep = 1;
  p.bfpart = 1;
  p.xch = xch_acquire(sizeof(float) * (size_t)T * dirs * p.nwg * (16 * H + 64) * p.rg, s);
  // self-tagged hand-off (fp32 partials through the L2 ring): the two ring
  // images start with tag 1 in every word (steps 0 and 1 publish tag 0)
  p.dtag = d.prec != kPrecBf16 && p.ring == 2 && p.xpd && T >= 2;
  if (p.dtag)
    KCTC_HIP_CHECK(hipMemsetAsync(p.xch, 0x01, sizeof(float) * 2 * (size_t)dirs * p.nwg * (16 * H + 64) * p.rg, s));
  p.e_sc1 = e_sc1 ? 1 : 0;  // dGates rows written through for a streaming consumer
  // bf16: dGates straight into the packed operands of the dx / dW / dR GEMMs
  // (no fp32 rows, no pack passes over them; KCTC_BF16_DIRECT=0: the fp32
  // rows and the pack kernels as in round 3), beside e_sc1's write-through rows when streamed
  if (bf16_direct(d, 6)) {
    p.dxr = reinterpret_cast<__bf16 *>(R0 + lay.pkxr);
    p.dxt = reinterpret_cast<__bf16 *>(R0 + lay.pkxt);
    p.eshift = bf16_io(d) ? 1 : 0;
    p.et = (d.mode == kGru || p.eshift) ? reinterpret_cast<__bf16 *>(R0 + lay.pket) : p.dxt;
    p.kbt64 = lay.kbt64;
    const size_t pitch = sizeof(__bf16) * lay.kbt64;
    const size_t rows = (size_t)NW * H;  // per direction
    if (lay.kbt64 > TN)  // the frame tail of every packed row stays zero
      KCTC_HIP_CHECK(hipMemset2DAsync(p.dxt + TN, pitch, 0, sizeof(__bf16) * (lay.kbt64 - TN), dirs * rows, s));
    if (p.eshift) {  // E^T shifted: direction 0 from TN - N on, direction 1 before N and from TN on
      KCTC_HIP_CHECK(hipMemset2DAsync(p.et + TN - N, pitch, 0, sizeof(__bf16) * (lay.kbt64 - TN + N), rows, s));
      KCTC_HIP_CHECK(hipMemset2DAsync(p.et + rows * lay.kbt64, pitch, 0, sizeof(__bf16) * N, rows, s));
      if (lay.kbt64 > TN)
        KCTC_HIP_CHECK(hipMemset2DAsync(p.et + rows * lay.kbt64 + TN, pitch, 0, sizeof(__bf16) * (lay.kbt64 - TN),
                                        rows, s));
    } else if (d.mode == kGru && lay.kbt64 > TN) {
      KCTC_HIP_CHECK(hipMemset2DAsync(p.et + TN, pitch, 0, sizeof(__bf16) * (lay.kbt64 - TN), dirs * rows, s));
    }
  }
  p.cmax = ws.at<unsigned>(ws.lay.cme);
  if (p.rg > 1)  // max over the row groups by atomicMax on the float bits
    KCTC_HIP_CHECK(hipMemsetAsync(p.cmax, 0, sizeof(unsigned) * 2 * dirs * NW * H, s));
}

// dx_l = sum_dir DX_dir W_dir on s after the recurrence (not streamed): packed
// bf16 (dxr: the dGates rows the recurrence wrote packed, or null), packed
// split-fp16, or (few gate columns) fp32
void dx_gemm(const RnnDesc &d, const RnnWs &ws, hipStream_t s, long TN, int l, const float *DX, __bf16 *dxr,
             const float *wl, long pls, float *dxl) {
  const int dirs = d.dirs, Din = d.din(l);
  const long G4 = (long)d.nw() * d.H;
  if (d.prec == kPrecBf16 && use_x3((int)G4)) {
    // dGates rows and W^T rows (columns of W) packed as bf16
    const int KB = (int)((G4 + 63) / 64);
    __bf16 *Ap = dxr ? dxr : ws.at<__bf16>(ws.lay.a), *Bp = ws.at<__bf16>(ws.lay.b);
    {
      ProfSpan ps(s, "x3_pack");
      if (!dxr) bf16_pack_rows(s, DX, (long)dirs * G4, (int)TN, (int)G4, Ap, dirs, G4, TN * KB * 64);
      for (int dir = 0; dir < dirs; dir++)
        bf16_pack_cols(s, wl + dir * pls, Din, (int)G4, Din, 0, Bp + (long)dir * Din * KB * 64);
    }
    for (int dir = 0; dir < dirs; dir++) {
      ProfSpan ps(s, "gemm_bwd_data");
      X3PArgs x;
      x.bf16 = true;
      x.M = (int)TN; x.N = Din; x.KB = KB;
      x.A = reinterpret_cast<const _Float16 *>(Ap + (long)dir * TN * KB * 64);
      x.B = reinterpret_cast<const _Float16 *>(Bp + (long)dir * Din * KB * 64);
      x.C = dxl; x.ldc = Din; x.beta = dir == 0 ? 0.f : 1.f;
      gemm_x3p(s, x);
    }
  } else if (use_x3((int)G4)) {
    const int KB = (int)((G4 + 31) / 32);
    _Float16 *Ap = ws.at<_Float16>(ws.lay.a), *Bp = ws.at<_Float16>(ws.lay.b);
    int *eA = ws.at<int>(ws.lay.ea), *eB = ws.at<int>(ws.lay.eb);
    unsigned *cm = ws.at<unsigned>(ws.lay.cm);
    {
      // dGates rows (frames, per direction) and W^T rows (input dims), packed over the gates
      ProfSpan ps(s, "x3_pack");
      x3p_pack_rows(s, DX, (long)dirs * G4, (int)TN, (int)G4, Ap, eA, 0.f, dirs, G4, TN * KB * 64, TN);
      for (int dir = 0; dir < dirs; dir++) {
        absmax_f32(s, wl + dir * pls, Din, (int)G4, Din, nullptr, cm);
        x3p_pack_cols(s, wl + dir * pls, Din, (int)G4, Din, 0, Bp + (long)dir * Din * KB * 64, eB + dir * Din, cm,
                      0.f);
      }
    }
    for (int dir = 0; dir < dirs; dir++) {
      ProfSpan ps(s, "gemm_bwd_data");
      X3PArgs x;
      x.M = (int)TN; x.N = Din; x.KB = KB;
      x.A = Ap + (long)dir * TN * KB * 64; x.eA = eA + (long)dir * TN;
      x.B = Bp + (long)dir * Din * KB * 64; x.eB = eB + dir * Din;
      x.C = dxl; x.ldc = Din; x.beta = dir == 0 ? 0.f : 1.f;
      gemm_x3p(s, x);
    }
  } else {
    for (int dir = 0; dir < dirs; dir++) {
      ProfSpan ps(s, "gemm_bwd_data");
      GemmArgs g;
      g.transA = false; g.transB = false;
      g.M = (int)TN; g.N = Din; g.K = (int)G4;
      g.A = DX + (long)dir * G4; g.lda = (long)dirs * G4;
      g.B = wl + dir * pls; g.ldb = Din;
      g.C = dxl; g.ldc = Din;
      g.beta = dir == 0 ? 0.f : 1.f;
      gemm_f32(s, g);
    }
  }
}
}  // namespace

int rnn_backward_data(const RnnDesc &d, hipStream_t s, int T, int N, const float *y,
                      const float *dy, const float *w, float *dx, void *workspace,
                      size_t ws_bytes, void *reserve, size_t res_bytes, unsigned *err,
                      hipStream_t overlap, RnnWgradStream *wgrad, const RnnPrepack *pre) {
  RecScope rec_scope;  // the side launches' residency gates (beside_recurrence)
  if (wgrad) wgrad->done = false;
  if (T <= 0 || N <= 0 || N > 16 * kMaxRT || d.H % 16) return KRNN_NOT_SUPPORTED;
  const RnnReserveLayout lay = rnn_reserve_layout(d, T, N);
  if (res_bytes < sizeof(float) * (size_t)lay.total) return KRNN_BAD_PARAM;
  const RecPlan pl = plan_rec(d, N, false);
  if (!pl) return KRNN_NOT_SUPPORTED;
  const RnnWs ws(d, T, N, workspace);
  if (ws_bytes < ws.bytes()) return KRNN_BAD_PARAM;
  const bool v6 = pl.ver == 6;
  const int dirs = d.dirs;
  const long TN = (long)T * N;
  float *res = static_cast<float *>(reserve);
  const float *dcur = dy;
  for (int l = d.layers - 1; l >= 0; l--) {
    float *R0 = res + lay.per_layer * l;
    const float *out = (l == d.layers - 1) ? y : R0 + lay.out;
    const LayerW lw = layer_w(d, l);
    const float *wl = w + lw.pl0;
    float *E = R0 + lay.E;
    float *DX = d.mode == kGru ? R0 + lay.DX : E;
    RecParams p = rec_params(d, pl, ws, T, N, wl, lw, R0, lay, const_cast<float *>(out), err, s);
    // dx_l = sum_dir DX_dir W_dir   (lower layer's dy, or the caller's dx)
    float *dxl = (l == 0) ? dx : res + lay.per_layer * (l - 1) + lay.dout;
    // streamed: computed on `overlap` while the recurrence runs, from its rows as they appear
    const bool streamed = dxl && overlap && v6 && bwd_dx_stream_ok(pl, d, l, T, N);
    // weight gradients streamed off this recurrence (the bottom component):
    // its dGates rows must be written through too
    const bool wstream = wgrad && wgrad->side && !dxl && v6 && !p.xpd && d.layers == 1 &&
                         wgrad_stream_shape(d, T, N) && wgrad_stream_ok(pl, d, T, N);
    bwd_rec_params(p, d, pl, ws, R0, lay, dcur, E, DX, streamed || wstream, s);
    const hipEvent_t fork = (streamed || wstream) ? fork_event(s) : nullptr;
    RegWord &rw = reg_of_device();
    if (v6) p.reg = rw.word;  // registration for the exchange's residency gate
    RecTrace tr;
    launch_planned(d, pl, false, p, tr, rec_scope, s);
    // counted once the launch is enqueued (a failed launch never raises the target)
    if (v6) rw.expected += (unsigned long long)pl.wgs;
    g_last_bwd_scratch_free = v6 ? pl.scratch_free : true;
    if (streamed) {
      launch_bwd_stream(d, p, l, w, dxl, ws, T, N, overlap, fork, err, d.layers == 1 ? pre : nullptr);
      join_stream(s, overlap);
    }
    if (wstream) launch_wgrad_stream(pl, d, p, fork, T, N, y, ws, reserve, err, *wgrad, s);
    if (v6) xch_release(s);
    tr.dump("bwd", s, pl.grid, p.nwg, T, dirs, pl.ver, p.xpd);
    if (dxl && !streamed) dx_gemm(d, ws, s, TN, l, DX, p.dxr, wl, lw.pls, dxl);
    dcur = dxl;
  }
  return KRNN_OK;
}

// ---------------------------------------------------------------------------
// host: backward weights (accumulates into dw, like cudnnRNNBackwardWeights)
// ---------------------------------------------------------------------------
namespace {
// One stacked layer of rnn_backward_weights: dW_dir += DX_dir^T in and
// dR_dir += E_dir(shifted)^T h_prev -- direction 0 pairs rows t >= 1 with out
// rows t - 1, direction 1 rows t <= T - 2 with out rows t + 1
struct WgradLayer {
  const RnnDesc &d;
  const RnnWs &ws;
  hipStream_t s;
  int T, N, l;
  const float *in, *out;  // the layer's input and output rows
  float *E, *DX;          // dGates (recurrent / input part; the same but for a GRU)
  float *dwl;             // the layer's gradient block
  long pls, roff;         // LayerW
  int max_blocks;
  long TN() const { return (long)T * N; }
  long G4() const { return (long)d.nw() * d.H; }
};

// bf16 weight GEMMs: the transposes packed along the frames as bf16
void wgrad_bf16(const WgradLayer &g, float *R0, const RnnReserveLayout &lay, const void *in_cols) {
  const RnnDesc &d = g.d;
  const RnnWs &ws = g.ws;
  hipStream_t s = g.s;
  const int H = d.H, dirs = d.dirs, Din = d.din(g.l), N = g.N;
  const long TN = g.TN(), G4 = g.G4(), ldg = dirs * G4, ldy = (long)dirs * H;
  const int KB = (int)((TN + 63) / 64);
  // the dGates transposes: written packed by the backward recurrence (bf16_direct)
  const bool pkd = bf16_direct(d, 6);
  // bf16_io: the forward wrote y^T packed (unshifted) and the backward
  // E^T shifted by one step; the input's columns may come packed from the
  // previous component's forward (in_cols)
  const bool io = bf16_io(d);
  const bool cols_in = g.l == 0 && in_cols != nullptr;
  __bf16 *DXt = pkd ? reinterpret_cast<__bf16 *>(R0 + lay.pkxt) : ws.at<__bf16>(ws.lay.a);
  __bf16 *Xt = cols_in ? static_cast<__bf16 *>(const_cast<void *>(in_cols)) : ws.at<__bf16>(ws.lay.b);
  __bf16 *Yt = io ? reinterpret_cast<__bf16 *>(R0 + lay.pkyc) : ws.at<__bf16>(ws.lay.c);
  __bf16 *Et = (d.mode == kGru || io)
                   ? (pkd ? reinterpret_cast<__bf16 *>(R0 + lay.pket) : DXt + (long)dirs * G4 * KB * 64)
                   : DXt;
  {
    ProfSpan ps(s, "x3_pack_w");
    if (!pkd) {
      bf16_pack_cols(s, g.DX, ldg, (int)TN, (int)(dirs * G4), 0, DXt);
      if (d.mode == kGru) bf16_pack_cols(s, g.E, ldg, (int)TN, (int)(dirs * G4), 0, Et);
    }
    if (!cols_in) bf16_pack_cols(s, g.in, Din, (int)TN, Din, 0, Xt);
    if (g.T > 1 && !io)
      for (int dir = 0; dir < dirs; dir++)
        bf16_pack_cols(s, g.out + (long)dir * H, ldy, (int)TN, H, dir == 0 ? N : -N, Yt + (long)dir * H * KB * 64);
  }
  {
    X3PArgs x;
    x.bf16 = true;
    x.M = (int)G4; x.N = Din; x.KB = KB;
    x.A = reinterpret_cast<const _Float16 *>(DXt); x.sA = G4 * KB * 64;
    x.B = reinterpret_cast<const _Float16 *>(Xt);
    x.C = g.dwl; x.ldc = Din; x.beta = 1.f;
    x.batch = dirs; x.sC = g.pls;
    x.split_k = x3p_pick_split((int)G4, Din, KB, dirs); x.ws = ws.split_slab();
    x.max_blocks = g.max_blocks; x.tile_counter = tile_counter(ws, kTileWordW, g.max_blocks);
    ProfSpan ps(s, "gemm_bwd_w");
    gemm_x3p(s, x);
  }
  if (g.T > 1) {
    X3PArgs x;
    x.bf16 = true;
    x.M = (int)G4; x.N = H; x.KB = KB;
    x.A = reinterpret_cast<const _Float16 *>(Et); x.sA = G4 * KB * 64;
    x.B = reinterpret_cast<const _Float16 *>(Yt); x.sB = (long)H * KB * 64;
    x.C = g.dwl + g.roff; x.ldc = H; x.beta = 1.f;
    x.batch = dirs; x.sC = g.pls;
    x.split_k = x3p_pick_split((int)G4, H, KB, dirs); x.ws = ws.split_slab();
    x.max_blocks = g.max_blocks; x.tile_counter = tile_counter(ws, kTileWordR, g.max_blocks);
    ProfSpan ps(s, "gemm_bwd_r");
    gemm_x3p(s, x);
  }
}

// fp32 weight GEMMs (few frames)
void wgrad_f32(const WgradLayer &g) {
  const RnnDesc &d = g.d;
  const int H = d.H, dirs = d.dirs, Din = d.din(g.l), N = g.N, G4 = (int)g.G4();
  const long ldg = (long)dirs * G4, ldy = (long)dirs * H;
  {
    GemmArgs w;
    w.transA = true; w.transB = false;
    w.M = G4; w.N = Din; w.K = (int)g.TN();
    w.A = g.DX; w.lda = ldg; w.B = g.in; w.ldb = Din;
    w.C = g.dwl; w.ldc = Din; w.beta = 1.f;
    w.batch = dirs; w.strideA = G4; w.strideB = 0; w.strideC = g.pls;
    w.split_k = gemm_pick_split(w.M, w.N, w.K, dirs);
    w.ws = g.ws.split_slab();
    w.max_blocks = g.max_blocks;
    w.tile_counter = tile_counter(g.ws, kTileWordW, g.max_blocks);
    ProfSpan ps(g.s, "gemm_bwd_w");
    gemm_f32(g.s, w);
  }
  if (g.T > 1) {
    GemmArgs r;
    r.transA = true; r.transB = false;
    r.M = G4; r.N = H; r.K = (int)((long)(g.T - 1) * N);
    r.A = g.E + (long)N * ldg; r.lda = ldg;
    r.B = g.out; r.ldb = ldy;
    r.C = g.dwl + g.roff; r.ldc = H; r.beta = 1.f;
    r.batch = dirs;
    r.strideA = (long)G4 - (long)N * ldg;        // dir 1: E + G4 (rows 0..T-2)
    r.strideB = (long)N * ldy + H;               // dir 1: y rows 1..T-1, cols H..
    r.strideC = g.pls;
    r.split_k = gemm_pick_split(r.M, r.N, r.K, dirs);
    r.ws = g.ws.split_slab();
    r.max_blocks = g.max_blocks;
    r.tile_counter = tile_counter(g.ws, kTileWordR, g.max_blocks);
    ProfSpan ps(g.s, "gemm_bwd_r");
    gemm_f32(g.s, r);
  }
}

// The packed operands of wgrad_x3: dGates^T (per-gate exponents), input^T
// (per-dim), the output^T shifted by one step per direction, E^T (GRU; else
// dGates^T again), each with its exponents
struct WgradCols {
  _Float16 *DXt, *Xt, *Yt, *Et;
  int *eDX, *eX, *eY, *eE;
  const unsigned *cme;  // the dGates column maxima a v6 backward recurrence left behind (else null)
  bool wpre;            // x^T and y^T came packed from the forward (RnnPrepack::wgrad)
};

// Two streams (s2, the bottom component's tail, where nothing else overlaps):
// input^T and output^T are packed (and dW then runs) on s2 while dGates^T is
// packed (and dR runs) on s: separate split slabs, tile counters and absmax
// scratch.  (LSTM: dR's dGates^T is dW's, E == DX.)
void pack_wgrad_two(const WgradLayer &g, const WgradCols &c, float in_bound, hipStream_t s2, hipEvent_t ev_dx,
                    hipEvent_t ev_y) {
  const RnnDesc &d = g.d;
  hipStream_t s = g.s;
  const int H = d.H, dirs = d.dirs, Din = d.din(g.l), N = g.N;
  const long TN = g.TN(), G4 = g.G4(), ldy = (long)dirs * H, KBt = (TN + 31) / 32;
  ProfSpan ps(s, "x3_pack_w");
  x3p_pack_cols(s, g.DX, dirs * G4, (int)TN, (int)(dirs * G4), 0, c.DXt, c.eDX, c.cme, 0.f);
  KCTC_HIP_CHECK(hipEventRecord(ev_dx, s));
  const bool xb = g.l == 0 && in_bound > 0.f;
  // absmax scratch of its own: the GRU-only E^T exponent array (free for an LSTM)
  unsigned *cmx = reinterpret_cast<unsigned *>(g.ws.at<int>(g.ws.lay.ed));
  if (!c.wpre) {
    if (!xb) absmax_f32(s2, g.in, Din, (int)TN, Din, nullptr, cmx);
    x3p_pack_cols(s2, g.in, Din, (int)TN, Din, 0, c.Xt, c.eX, cmx, xb ? in_bound : 0.f);
    for (int dir = 0; dir < dirs; dir++)
      x3p_pack_cols(s2, g.out + (long)dir * H, ldy, (int)TN, H, dir == 0 ? N : -N, c.Yt + (long)dir * H * KBt * 64,
                    c.eY + dir * H, nullptr, 1.f);
  }
  KCTC_HIP_CHECK(hipEventRecord(ev_y, s2));
  KCTC_HIP_CHECK(hipStreamWaitEvent(s2, ev_dx, 0));
  KCTC_HIP_CHECK(hipStreamWaitEvent(s, ev_y, 0));
}

// One stream; beside another component's pinned recurrence the packs keep off its XCDs
void pack_wgrad_one(const WgradLayer &g, const WgradCols &c, float in_bound, bool beside) {
  const RnnDesc &d = g.d;
  const RnnWs &ws = g.ws;
  hipStream_t s = g.s;
  const int H = d.H, dirs = d.dirs, Din = d.din(g.l), N = g.N, l = g.l;
  const long TN = g.TN(), G4 = g.G4(), ldg = dirs * G4, ldy = (long)dirs * H, KBt = (TN + 31) / 32;
  unsigned *cm = ws.at<unsigned>(ws.lay.cm);
  ProfSpan ps(s, "x3_pack_w");
  // (x3p_pack_cols avoid)
  const unsigned *av = beside ? rnn_pinned_xcds() : nullptr;
  const int nx = std::max(1, rnn_usable_cus() / kCusPerXcd);
  // their item counters: flag words kPackWord.. (this component's
  // recurrences, which use the flag words, are done)
  int *pc = reinterpret_cast<int *>(ws.flags() + kPackWord);
  if (av) KCTC_HIP_CHECK(hipMemsetAsync(pc, 0, sizeof(int) * kPackWords, s));
  if (!c.cme) absmax_f32(s, g.DX, ldg, (int)TN, (int)(dirs * G4), nullptr, cm);
  x3p_pack_cols(s, g.DX, ldg, (int)TN, (int)(dirs * G4), 0, c.DXt, c.eDX, c.cme ? c.cme : cm, 0.f, 1, 0, 0, 0, 0, av,
                nx, pc);
  if (d.mode == kGru) {
    if (!c.cme) absmax_f32(s, g.E, ldg, (int)TN, (int)(dirs * G4), nullptr, cm);
    x3p_pack_cols(s, g.E, ldg, (int)TN, (int)(dirs * G4), 0, c.Et, c.eE, c.cme ? c.cme + dirs * G4 : cm, 0.f, 1, 0, 0,
                  0, 0, av, nx, pc + 1);
  }
  if (c.wpre) return;
  const bool xb = (l > 0 && bounded_out(d)) || (l == 0 && in_bound > 0.f);
  if (!xb) absmax_f32(s, g.in, Din, (int)TN, Din, nullptr, cm);
  x3p_pack_cols(s, g.in, Din, (int)TN, Din, 0, c.Xt, c.eX, cm, xb ? (l > 0 ? 1.f : in_bound) : 0.f, 1, 0, 0, 0, 0, av,
                nx, pc + 2);
  if (g.T > 1) {
    if (!bounded_out(d)) absmax_f32(s, g.out, ldy, (int)TN, (int)ldy, nullptr, cm);
    for (int dir = 0; dir < dirs; dir++)
      x3p_pack_cols(s, g.out + (long)dir * H, ldy, (int)TN, H, dir == 0 ? N : -N, c.Yt + (long)dir * H * KBt * 64,
                    c.eY + dir * H, bounded_out(d) ? nullptr : cm + dir * H, bounded_out(d) ? 1.f : 0.f, 1, 0, 0, 0,
                    0, av, nx, pc + 3 + dir);
  }
}

// split-fp16 weight GEMMs on operands packed over the frames (all frames: the
// shifted-out ones are zero in the packed output^T).  v6b: the layer's
// backward ran v6.
void wgrad_x3(const WgradLayer &g, bool v6b, float in_bound, hipStream_t s2, bool beside, const RnnPrepack *pre) {
  const RnnDesc &d = g.d;
  const RnnWs &ws = g.ws;
  const PackLay &pl = ws.lay;
  hipStream_t s = g.s;
  const int H = d.H, dirs = d.dirs, Din = d.din(g.l), T = g.T;
  const long TN = g.TN(), G4 = g.G4();
  const int KBt = (int)((TN + 31) / 32);
  WgradCols c;
  // x^T and y^T packed by the forward, else here
  c.wpre = pre && pre->wdone && pre->wev && d.layers == 1 && T > 1;
  c.DXt = ws.at<_Float16>(pl.a);
  c.Xt = ws.at<_Float16>(c.wpre ? pl.xt : pl.b);
  c.Yt = ws.at<_Float16>(c.wpre ? pl.yt : pl.c);
  c.Et = d.mode == kGru ? c.DXt + (long)dirs * G4 * KBt * 64 : c.DXt;
  c.eDX = ws.at<int>(pl.ea);
  c.eX = ws.at<int>(c.wpre ? pl.ext : pl.eb);
  c.eY = ws.at<int>(c.wpre ? pl.eyt : pl.ec);
  c.eE = d.mode == kGru ? ws.at<int>(pl.ed) : c.eDX;
  c.cme = v6b ? ws.at<unsigned>(pl.cme) : nullptr;
  if (c.wpre) KCTC_HIP_CHECK(hipStreamWaitEvent(s, pre->wev, 0));
  // (the GRU's E^T pack stays on one stream)
  const bool two = s2 && c.cme && d.mode == kLstm && d.layers == 1 && T > 1 && env_int("KCTC_WGRAD_2S", 1);
  hipStream_t sx = two ? s2 : s;  // stream of the input / output packs and of dW
  hipEvent_t ev_dx = nullptr, ev_y = nullptr;
  if (two) {
    KCTC_HIP_CHECK(hipEventCreateWithFlags(&ev_dx, hipEventDisableTiming));
    KCTC_HIP_CHECK(hipEventCreateWithFlags(&ev_y, hipEventDisableTiming));
    join_stream(s2, s);
    pack_wgrad_two(g, c, in_bound, s2, ev_dx, ev_y);
  } else {
    pack_wgrad_one(g, c, in_bound, beside);
  }
  // beside another component's pinned backward recurrence: dW and dR as
  // one launch on the CUs it leaves (gemm_x3p_pair; configs[1]: the side
  // stream fell one GEMM per layer behind, 4 ms of weight GEMMs after the
  // last recurrence)
  const bool pair = beside && !two && T > 1 && x3p_use_256((int)G4, Din) && x3p_use_256((int)G4, H) &&
                    g.max_blocks > 0;
  X3PArgs xw;
  xw.M = (int)G4; xw.N = Din; xw.KB = KBt;
  xw.A = c.DXt; xw.eA = c.eDX; xw.sA = G4 * KBt * 64; xw.seA = G4;
  xw.B = c.Xt; xw.eB = c.eX;
  xw.C = g.dwl; xw.ldc = Din; xw.beta = 1.f;
  xw.batch = dirs; xw.sC = g.pls;
  xw.split_k = x3p_pick_split((int)G4, Din, KBt, dirs);
  // concurrent with dR: its own split slab past dR's (none when dR is not
  // split: the slabs reserve room for dR only for a split > 1)
  const long sR = x3p_pick_split((int)G4, H, KBt, dirs);
  xw.ws = (two || pair) && sR > 1 ? ws.split_slab() + (sR * dirs * G4 * H + 63) / 64 * 64 : ws.split_slab();
  xw.max_blocks = g.max_blocks; xw.tile_counter = tile_counter(ws, kTileWordW, g.max_blocks);
  if (pair) {
    xw.max_blocks = 192;
    xw.avoid_word = rnn_pinned_xcds();
    xw.avoid_xcds = std::max(1, rnn_usable_cus() / kCusPerXcd);
  } else {
    ProfSpan ps(sx, "gemm_bwd_w");
    gemm_x3p(sx, xw);
  }
  if (T > 1) {
    ProfSpan ps(s, "gemm_bwd_r");
    X3PArgs x;
    x.M = (int)G4; x.N = H; x.KB = KBt;
    x.A = c.Et; x.eA = c.eE; x.sA = G4 * KBt * 64; x.seA = G4;
    x.B = c.Yt; x.eB = c.eY; x.sB = (long)H * KBt * 64; x.seB = H;
    x.C = g.dwl + g.roff; x.ldc = H; x.beta = 1.f;
    x.batch = dirs; x.sC = g.pls;
    x.split_k = x3p_pick_split((int)G4, H, KBt, dirs); x.ws = ws.split_slab();
    x.max_blocks = g.max_blocks; x.tile_counter = tile_counter(ws, kTileWordR, g.max_blocks);
    if (pair) gemm_x3p_pair(s, xw, x);  // xw's tile counter, block count and avoid word
    else gemm_x3p(s, x);
  }
  if (two) {
    join_stream(s, s2);
    (void)hipEventDestroy(ev_dx);
    (void)hipEventDestroy(ev_y);
  }
}
}  // namespace

int rnn_backward_weights(const RnnDesc &d, hipStream_t s, int T, int N, const float *x,
                         const float *y, void *workspace, size_t ws_bytes, float *dw,
                         void *reserve, size_t res_bytes, int max_blocks, float in_bound, hipStream_t s2,
                         const void *in_cols, bool beside, const RnnPrepack *pre) {
  const RnnReserveLayout lay = rnn_reserve_layout(d, T, N);
  if (res_bytes < sizeof(float) * (size_t)lay.total) return KRNN_BAD_PARAM;
  const RnnWs ws(d, T, N, workspace);
  if (ws_bytes < ws.bytes()) return KRNN_BAD_PARAM;
  const RecPlan plb = plan_rec(d, N, false);  // the backward recurrence that left dGates and bias partials
  float *res = static_cast<float *>(reserve);
  // K = frames: large (also for a 40-dim input: 0.8 ms/step over fp32).
  // A bf16 backward that wrote its dGates packed (bf16_direct) left no fp32
  // rows: its packed operands are the only ones, however few the frames
  // (under 128 frames the fp32 GEMMs would read rows nobody had written)
  const bool x3 = use_x3((int)((long)T * N)) || bf16_direct(d, 6);
  for (int l = 0; l < d.layers; l++) {
    float *R0 = res + lay.per_layer * l;
    const LayerW lw = layer_w(d, l);
    float *E = R0 + lay.E;
    const WgradLayer g{d, ws, s, T, N, l,
                       l == 0 ? x : res + lay.per_layer * (l - 1) + lay.out,
                       (l == d.layers - 1) ? y : R0 + lay.out,
                       E, d.mode == kGru ? R0 + lay.DX : E,
                       dw + lw.pl0, lw.pls, lw.roff, max_blocks};
    if (x3 && d.prec == kPrecBf16) wgrad_bf16(g, R0, lay, in_cols);
    else if (x3) wgrad_x3(g, plb.ver == 6, in_bound, s2, beside, pre);
    else wgrad_f32(g);
    wgrad_bias(plb, d, s, T, N, dw, reserve, l);
  }
  return KRNN_OK;
}

}  // namespace kctc
