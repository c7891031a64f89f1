// rnn.hip -- cuDNN-v5 compatible LSTM / GRU / RELU / TANH layers for gfx950.
//
// Replaces cudnnRNNForwardTraining / BackwardData / BackwardWeights as the
// reference calls them (src/cudamatrix/cudnn-recurrent.cc:13-102 through
// src/nnet2/nnet-cudnn-component.cc:508-614).  The host side is cut by pass;
// none of these units defines a kernel:
//   rnn.hip          the parameter layout (RnnDesc), rnn_set_precision,
//                    rnn_packed_output, and what every pass shares: the
//                    recurrence launch (rec_params, launch_planned, RecTrace),
//                    the exchange pool, fork / join of side streams, the entry
//                    checks (RnnCall), the packs and packed products that
//                    exist for both precisions
//   rnn_stream.hip   what may stream off a running v6 recurrence and the
//                    streamed launches: the next component's projection
//                    (launch_chain_proj / _rows), the dx GEMM
//                    (launch_bwd_stream), the chunked weight gradients
//                    (launch_wgrad_stream)
//   rnn_fwd.hip      rnn_forward_training, rnn_forward_inference_seq,
//                    rnn_forward_training_seq (and the length-aware
//                    training's buffer layout, SeqTrainLay)
//   rnn_bwd_data.hip rnn_backward_data, rnn_backward_data_seq
//   rnn_wgrad.hip    rnn_backward_weights, rnn_backward_weights_seq
//   rnn_host.h       the declarations these units share
// Which recurrence runs and where the workspace's parts lie: rnn_plan.hip
// (plan_rec, RnnWs); what may run beside a recurrence: rec_gate.hip; the
// kernels: rec6_fwd.hip, rec6_bwd.hip, rec_generic.hip, rec_common.h.
// Per stacked layer:
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
//     for the streamed GEMMs outside the XCD (rnn_stream.hip epoch_lines).
// Every spin is bounded (3 s); a timeout sets the device error word, every
// workgroup drains out and the train step fails loudly.
// One generic kernel pair (fp32 MFMA, all-gather of h / dGates per step through
// epoch flags, XCD-slot block mapping where the shape has whole slots) runs
// the shapes v6 does not compile (RELU / TANH, other H).
//
// Semantics follow cuDNN v5 as used by CuDNNRecurrentComponent: hx = cx = 0,
// dhy = dcy = 0 (SetBufferZero, nnet-cudnn-component.cc:494-506), all N
// sequences run the full T steps (no masking), weights in the opaque layout of
// nnet-cudnn-component.cc:327-413 (see RnnDesc::lin_offset).
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

#include "rnn_host.h"

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

LayerW layer_w(const RnnDesc &d, int l) {
  LayerW lw;
  lw.pl0 = d.lin_offset(l * d.dirs, 0, false);
  lw.pls = d.pl_size(l);
  lw.roff = d.lin_offset(l * d.dirs, d.nw(), false) - lw.pl0;
  lw.bW = d.lin_offset(l * d.dirs, 0, true) - lw.pl0;
  lw.bR = d.lin_offset(l * d.dirs, d.nw(), true) - lw.pl0;
  return lw;
}

bool range_ok(const RnnDesc &d, int T, int N) { return T > 0 && N > 0 && N <= 16 * kMaxRT && d.H % 16 == 0; }

bool RecTrace::arm(const char *tag, int grid) {
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
void RecTrace::dump(const char *tag, hipStream_t s, int grid, int nwg, int T, int dirs, int ver, int xpd) {
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

// Per-device exchange pool of the v6 backward: one step image per time step,
// never reused within a launch (T x dirs x nwg x H x Npad floats, 4.2 GB for
// BLSTM-512 N=16 T=2000).  Library-owned so that the components of a network
// share it; launches on one device are ordered through its event.
struct XchPool {
  void *p = nullptr;
  size_t bytes = 0;
  hipEvent_t ev = nullptr;
};
static std::mutex g_xch_mu;
static XchPool g_xch[64];

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
// after the recurrence's flag reset, and not before every workgroup of it is
// resident: a block parked on a CU of an XCD the recurrence is pinned to
// before its last workgroup got there would keep it out (seen once as a 3-s
// stream-wait timeout, error 0x2)
void go_beside(hipStream_t side, hipEvent_t fork) {
  if (fork) KCTC_HIP_CHECK(hipStreamWaitEvent(side, fork, 0));
  beside_recurrence(side);
}

PackAvoid avoid_pair() { return {rnn_pinned_xcds(), std::max(1, rnn_usable_cus() / kCusPerXcd), nullptr}; }

// ---------------------------------------------------------------------------
// packs and packed products that exist for both precisions
// ---------------------------------------------------------------------------
void pack_rows(bool bf, hipStream_t s, const float *X, long ldx, int R, int K, _Float16 *out, int *e, float bound,
               int batch, long sX, long sOut, long sE) {
  if (bf) bf16_pack_rows(s, X, ldx, R, K, reinterpret_cast<__bf16 *>(out), batch, sX, sOut);
  else x3p_pack_rows(s, X, ldx, R, K, out, e, bound, batch, sX, sOut, sE);
}
void pack_cols(bool bf, hipStream_t s, const float *X, long ldx, int R, int Cn, int shift, _Float16 *out, int *e,
               unsigned *cm, float bound, PackAvoid av) {
  if (bf) return bf16_pack_cols(s, X, ldx, R, Cn, shift, reinterpret_cast<__bf16 *>(out));
  if (!(bound > 0.f)) absmax_f32(s, X, ldx, R, Cn, nullptr, cm);
  x3p_pack_cols(s, X, ldx, R, Cn, shift, out, e, cm, bound > 0.f ? bound : 0.f, av);
}
void pack_shifted_y(bool bf, hipStream_t s, const float *out, int dirs, int H, long TN, int N, _Float16 *Yt, int *eY,
                    const unsigned *cm, PackAvoid av) {
  const long ldy = (long)dirs * H, sY = (long)H * kblocks(bf, TN) * 64;
  for (int dir = 0; dir < dirs; dir++) {
    const float *yd = out + (long)dir * H;
    const int shift = dir == 0 ? N : -N;
    if (bf)
      bf16_pack_cols(s, yd, ldy, (int)TN, H, shift, reinterpret_cast<__bf16 *>(Yt) + dir * sY);
    else
      x3p_pack_cols(s, yd, ldy, (int)TN, H, shift, Yt + dir * sY, eY + dir * H, cm ? cm + dir * H : nullptr,
                    cm ? 0.f : 1.f, av.counter ? av.at(dir) : av);
  }
}

X3PArgs packed_product(bool bf, int M, int N, int KB, const _Float16 *A, const int *eA, const _Float16 *B,
                       const int *eB, float *C, long ldc) {
  X3PArgs x;
  x.bf16 = bf;
  x.M = M; x.N = N; x.KB = KB;
  x.A = A; x.B = B;
  if (!bf) { x.eA = eA; x.eB = eB; }
  x.C = C; x.ldc = ldc;
  return x;
}

X3PArgs proj_product(const RnnDesc &d, const RnnWs &ws, hipStream_t s, long TN, int l, const float *wl, int KB,
                     float *G) {
  const bool bf = d.prec == kPrecBf16;
  const int Gn = d.nw() * d.H, Din = d.din(l);
  const LayerW lw = layer_w(d, l);
  _Float16 *Bp = ws.at<_Float16>(ws.lay.b);
  int *eB = ws.at<int>(ws.lay.eb);
  pack_rows(bf, s, wl, Din, Gn, Din, Bp, eB, 0.f, d.dirs, lw.pls, (long)Gn * KB * 64, Gn);
  X3PArgs x = packed_product(bf, (int)TN, Gn, KB, nullptr, nullptr, Bp, eB, G, (long)d.dirs * Gn);
  x.bias = wl + lw.bW;
  x.bias2 = d.mode == kGru ? nullptr : wl + lw.bR;
  x.batch = d.dirs; x.sB = (long)Gn * KB * 64; x.seB = bf ? 0 : Gn; x.sC = Gn; x.sBias = lw.pls;
  return x;
}

void pack_dx_wt(const RnnDesc &d, hipStream_t s, int l, const float *wl, int KB, _Float16 *Bp, int *eB, unsigned *cm,
                long cm_dir) {
  const int G4 = d.nw() * d.H, Din = d.din(l);
  const long pls = d.pl_size(l);
  for (int dir = 0; dir < d.dirs; dir++)
    pack_cols(d.prec == kPrecBf16, s, wl + dir * pls, Din, G4, Din, 0, Bp + (long)dir * Din * KB * 64, eB + dir * Din,
              cm + dir * cm_dir, 0.f);
}

}  // namespace kctc
