// rnn.h -- cuDNN-v5-compatible recurrent layer on gfx950 (internal C++ API).
// Replaces cudnnRNNForwardTraining / BackwardData / BackwardWeights as wrapped
// by src/cudamatrix/cudnn-recurrent.cc:13-102 of the reference.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace kctc {

enum RnnMode { kRelu = 0, kTanh = 1, kLstm = 2, kGru = 3 };

inline int rnn_nw(int mode) { return mode == kLstm ? 4 : mode == kGru ? 3 : 1; }

struct RnnDesc {
  int mode = kLstm, D = 0, H = 0, layers = 1, dirs = 2;
  // products of the recurrences and gate GEMMs: 0 fp32-class (split-fp16
  // pairs, fp32 accumulation), 1 bf16 (fp32 accumulation, fp32 master weights)
  int prec = 0;
  // bf16 only, latched by rnn_set_precision (not re-read per call: the reserve
  // layout must not change between the size query, the forward and the
  // backward): the recurrences write their GEMM operands packed (pk) and, one
  // layer bidirectional, the forward its output too (pkio)
  int pk = 1, pkio = 1;
  int nw() const { return rnn_nw(mode); }
  int din(int layer) const { return layer == 0 ? D : dirs * H; }
  // floats of one pseudo-layer block [W | R | bW | bR] of stacked layer `layer`
  long pl_size(int layer) const {
    long n = nw();
    return n * H * (long)din(layer) + n * H * (long)H + 2 * n * H;
  }
  long params_size() const;
  // float offset of lin layer `lin` (matrix or bias) of pseudo-layer p = layer*dirs + dir
  long lin_offset(int p, int lin, bool bias) const;
};

// Per-layer regions of the training reserve (floats), kept from forward to
// backward exactly like cuDNN's reserveSpace.
struct RnnReserveLayout {
  long G, aux, E, DX, bias, out, dout, per_layer, total;
  // bf16 precision: the backward recurrence's packed bf16 dGates operands
  // (RecParams::dxr / dxt / et; float offsets, 0 bytes otherwise), frames
  // padded to kbt64 per packed row
  long pkxr, pkxt, pket, kbt64;
  // bf16, one layer, bidirectional: the forward's packed bf16 copies of its
  // output (rows [T*N][2H], columns [2H][kbt64]); see rnn_packed_output
  long pkyr, pkyc;
};
RnnReserveLayout rnn_reserve_layout(const RnnDesc &d, int T, int N);
// set d.prec and latch the packed-operand switches (KCTC_BF16_DIRECT /
// KCTC_BF16_IO, both on by default) into d.pk / d.pkio
void rnn_set_precision(RnnDesc &d, int prec);
size_t rnn_workspace_bytes(const RnnDesc &d, int T, int N);

// CU budget of the persistent kernels.  A v6 recurrence needs
// all of its workgroups resident at once (one per CU, >= 96 KB LDS) and the
// streamed GEMMs' persistent blocks (one per CU as well) spin on its flags,
// so everything that may hold a CU beside them has to fit:
//   recurrence WGs + streamed blocks + comm CUs + 16 (margin) <= usable CUs.
// `cus`: the CUs this process may use (0: the device's; a smaller number
// when ranks share a device through CU-masked streams); `comm`: CUs the
// gradient exchange's kernels (RCCL, capped by maxCTAs) may hold during a
// backward pass.  Streaming is switched off when fewer than 8 blocks fit.
void rnn_set_cu_budget(int cus, int comm);
int rnn_usable_cus();
int rnn_comm_cus();
// test hook (test_hooks.h kctc_test_rec6_select): cfg = {U, nth, rg, gs,
// variant} of the v6 recurrence that (d, N, fwd) runs (zeros: not a v6 shape)
// and its kernel (nullptr then); nothing is launched
const void *rnn_rec6_select(const RnnDesc &d, int N, bool fwd, int cfg[5]);
// test hook (test_hooks.h kctc_test_rec_plan): the whole plan of the
// recurrence that (d, N, fwd) runs, any version: plan = {version (6 / 4 / 3;
// 0: not supported, the rest zeros), U, grid (workgroups), threads per
// workgroup, dynamic LDS bytes, XCDs a pinned v6 launch occupies (bit mask),
// workgroups per (row group, direction), RecParams::xpd}; nothing is launched
void rnn_rec_plan(const RnnDesc &d, int N, bool fwd, long plan[8]);
// test hook (test_hooks.h kctc_test_rnn_colmax_offset): byte offset, in the
// workspace of (d, T, N), of the dGates column maxima a v6 backward
// recurrence leaves ([2][dirs][nw H] float bits: DX, then the GRU's E)
size_t rnn_ws_colmax_offset(const RnnDesc &d, int T, int N);

// Residency gate of the gradient exchange.  Every workgroup
// of a v6 backward recurrence adds 1 to a per-device 64-bit registration
// counter when it starts; rnn_bwd_registrations() is the value it reaches
// once all backward recurrences enqueued so far on this device are resident.
// rnn_comm_gate(s, target) enqueues on s a gate kernel that returns once the
// counter has reached `target` (after 10 s it gives up and flags a gate
// timeout in the device word).  A gate is 8 one-wave blocks, one per XCD;
// a block on an XCD a recurrence is pinned to leaves (unless it is the last
// one waiting), so that no gate wave holds a CU a workgroup of that
// recurrence needs -- a workgroup that takes a CU's whole register file
// cannot be placed beside one (rec_gate.hip gate_kernel).  An exchange
// that runs its kernels only behind such a gate -- i.e. only while the
// backward recurrence launched last is fully resident -- and makes the next
// recurrence launch wait for them declares rnn_set_comm_gated(true): the
// backward recurrences then stay XCD-pinned with an exchange configured.
unsigned long long rnn_bwd_registrations();
// false when the backward recurrence this thread enqueued last uses scratch:
// nothing may then be queued beside it (rnn_plan.hip rec6_scratch_free), so the
// exchange waits for its end instead of its residency
bool rnn_last_bwd_scratch_free();
void rnn_comm_gate(hipStream_t s, unsigned long long target);
// s waits until the v6 launch whose flag area is `flags` has `target`
// workgroups resident (its own residency count; the same gate kernel, its
// blocks leaving on the XCDs that launch runs on)
void rnn_resident_gate(hipStream_t s, const unsigned *flags, unsigned target);
// Launches beside a running recurrence.  Every v6 recurrence counts its
// resident workgroups in its own flag area (kResWord, zeroed with the flags
// before the launch).  Each kernel that the RNN host puts on another stream while
// that recurrence runs -- the streamed GEMMs, the wgrad chunk gates, the
// forward-time packs -- is enqueued behind a gate kernel waiting for that count
// (rec_gate.hip beside_recurrence): nothing there can take a CU before every
// workgroup of the recurrence holds its own, so a consumer spinning on the
// recurrence's progress cannot keep a producer workgroup out.  The host
// refuses a streaming launch (gemm_x3p with producer.lines,
// gemm_x3p_bwd_stream) on a stream that has not passed the gate of the
// recurrence this thread has in flight: rnn_side_gated(s) is false then.
bool rnn_side_gated(hipStream_t s);
// device word: bit x set once an XCD-pinned backward recurrence ran on XCD x
// (never cleared; GEMMs launched beside one avoid those XCDs, X3PArgs::avoid_word)
const unsigned *rnn_pinned_xcds();
void rnn_set_comm_gated(bool on);
bool rnn_comm_gated();

// Status codes of the RNN ABI (include/kaldi_rnn.h)
enum { KRNN_OK = 0, KRNN_BAD_PARAM = 1, KRNN_NOT_SUPPORTED = 2, KRNN_EXEC_FAILED = 3,
       KRNN_TIMEOUT = 4 };

// All calls are stream-ordered; `err` is a device word (0 = ok) that the
// persistent kernels set on a bounded-spin timeout.
// Forward chaining of stacked components: the NEXT RNN component's layer-0
// input projection (the x3 GEMM of this call's output y) is computed on
// `side` while this call's last recurrence is still running, reading the
// recurrence's exchange images in place as their rows get published
// (gemm_x3p streaming mode).  The fork / join with `s` happens inside; `done`
// tells the caller whether the chain was taken -- if so it passes
// input_projected = true to the next component's forward, which then skips
// its layer-0 projection.
struct RnnFwdChain {
  const RnnDesc *d = nullptr;   // the consumer
  const float *w = nullptr;     // its parameters
  void *workspace = nullptr;    // its workspace / reserve (rnn_workspace_bytes, rnn_reserve_layout)
  size_t ws_bytes = 0;
  void *reserve = nullptr;
  size_t res_bytes = 0;
  hipStream_t side = nullptr;
  bool done = false;
};
// in_rows (nullable): the input already packed as bf16 rows [T*N][D] (the
// previous component's rnn_packed_output), used by a bf16 input projection
// instead of packing x.
// The backward's streamed dx GEMM reads W's columns packed (split-fp16 /
// bf16 rows of W^T).  W does not change between a training step's forward and
// backward, so rnn_forward_training packs them on `stream` while its own
// recurrence runs (CUs it leaves idle) into the workspace and records `ev`;
// rnn_backward_data then starts its streamed GEMM at once instead of behind
// the packs.  The caller owns ev and passes the same struct to the backward
// only while the parameters are unchanged (done: set by the forward).
struct RnnPrepack {
  hipStream_t stream = nullptr;
  hipEvent_t ev = nullptr;
  bool done = false;
  // the weight GEMMs' input^T and output^T (x and y packed along the frames,
  // one-layer split-fp16 components with bounded x and y): packed on `stream`
  // by the forward -- x beside its recurrence, y after it -- instead of on the
  // backward's side stream, where the CUs beside the next component's
  // recurrence are short (wev: recorded after both; wdone: packed)
  hipEvent_t wev = nullptr;
  bool dx = true;        // W^T (ev / done) requested
  bool wgrad = false;    // requested
  float in_bound = 0.f;  // |x| <= in_bound (> 0 required)
  bool wdone = false;
};
struct RnnFwdOpts {
  RnnFwdChain *chain = nullptr;
  bool input_projected = false;   // layer 0's projection is in the reserve (the previous component's chain)
  const void *in_rows = nullptr;
  RnnPrepack *pre = nullptr;
};
int rnn_forward_training(const RnnDesc &d, hipStream_t s, int T, int N, const float *x,
                         const float *w, float *y, void *workspace, size_t ws_bytes,
                         void *reserve, size_t res_bytes, unsigned *err, const RnnFwdOpts &o = {});
// Length-aware inference: N sequences of host lengths seq_lengths[n] in
// [1, T] (read before the call returns; KRNN_BAD_PARAM otherwise) run as one
// batch, each with the result it would get alone with hx = cx = 0:
//   y[t,n,:] = the layer's output for x[0:len[n], n] at frame t   (t < len[n])
//   y[t,n,:] = 0                                                  (t >= len[n])
// Rows t >= len[n] of x may hold anything.  The recurrences are the training
// forward's, unchanged: per stacked layer the reverse direction's columns of
// the projected gates G are shifted right by T - len[n] frames (seq_align.hip)
// so that it meets frame len[n]-1 with zero state, and its output is shifted
// back.  None of the streamed hand-overs (RnnFwdChain, in_rows) is used: they
// read un-shifted images.  workspace / reserve as rnn_forward_training;
// seq_buffer: rnn_seq_buffer_bytes(d, T, N) more bytes.
size_t rnn_seq_buffer_bytes(const RnnDesc &d, int T, int N);
int rnn_forward_inference_seq(const RnnDesc &d, hipStream_t s, int T, int N, const int *seq_lengths, const float *x,
                              const float *w, float *y, void *workspace, size_t ws_bytes, void *reserve,
                              size_t res_bytes, void *seq_buffer, size_t seq_bytes, unsigned *err);
// Length-aware training: the three passes with the semantics above, so that
//   y[:len[n], n], dx[:len[n], n]  are what sequence n gets run alone (N = 1, T = len[n]),
//   dw                            accumulates the SUM over n of those runs' gradients,
//   y and dx rows t >= len[n]     are +0 (rows t >= len[n] of x and dy may hold anything finite).
// The recurrence kernels are unchanged.  Forward: as the inference call, and
// every stacked layer's output is kept in the shifted frame for the backward
// recurrence.  Backward data: dy enters aligned like G (forward columns
// masked, reverse columns shifted right; seq_align_dy); with dh = dc = 0
// entering a padding step and dy = 0 on it every cell's backward yields zero
// gate gradients and passes zero on; the recurrence writes its dGates images
// into scratch and one launch shifts them back into the reserve
// (seq_unalign_dgates), where the dx GEMM and the weight GEMMs read them as
// ever.  Backward weights: un-shifted images only -- E / DX, the caller's y,
// the masked copy of x in the reserve -- since both E and y are zero on
// padding rows the one-step pairing of dR stays right (the shifted y holds
// whatever the recurrence computed on padding rows: unbounded for RELU).
// The same seq_lengths go to all three calls.  None of the streamed
// hand-overs is used (RnnFwdChain, in_rows, RnnPrepack, the streamed dx GEMM,
// RnnWgradStream): they read un-shifted step images.  fp32-class precision
// only: a bf16 descriptor returns KRNN_NOT_SUPPORTED (its backward writes the
// dGates packed, there are no fp32 rows to un-shift).  Workspace and reserve:
// rnn_seq_train_workspace_bytes / rnn_seq_train_reserve_bytes; the workspace
// must be the same from rnn_backward_data_seq to rnn_backward_weights_seq, as
// for the plain calls.
size_t rnn_seq_train_workspace_bytes(const RnnDesc &d, int T, int N);
size_t rnn_seq_train_reserve_bytes(const RnnDesc &d, int T, int N);
int rnn_forward_training_seq(const RnnDesc &d, hipStream_t s, int T, int N, const int *seq_lengths, const float *x,
                             const float *w, float *y, void *workspace, size_t ws_bytes, void *reserve,
                             size_t res_bytes, unsigned *err);
int rnn_backward_data_seq(const RnnDesc &d, hipStream_t s, int T, int N, const int *seq_lengths, const float *y,
                          const float *dy, const float *w, float *dx, void *workspace, size_t ws_bytes,
                          void *reserve, size_t res_bytes, unsigned *err);
struct RnnWgradOpts;
// (of o: max_blocks, in_bound, s2 and beside; in_cols and pre are not used)
int rnn_backward_weights_seq(const RnnDesc &d, hipStream_t s, int T, int N, const int *seq_lengths, const float *x,
                             const float *y, void *workspace, size_t ws_bytes, float *dw, void *reserve,
                             size_t res_bytes, const RnnWgradOpts &o);
// bf16 one-layer bidirectional components: the forward recurrence also writes
// its output as packed bf16 rows [T*N][2H] and columns [2H][kbt64] into the
// reserve (the GEMM operands the next component's projection / dW and this
// component's dR read).  Pointers valid after rnn_forward_training of (T, N)
// on this reserve; false (nullptrs) for other components.
bool rnn_packed_output(const RnnDesc &d, int T, int N, void *reserve, const void **rows, const void **cols);
// Weight gradients of a one-layer bidirectional split-fp16 LSTM computed off
// its RUNNING backward recurrence (the bottom component, which has no dx to
// stream): the frames are cut into `chunks` per direction in the order the
// recurrence finishes them (direction 0 from the last frame down, direction
// 1 from the first up); on `side`, a one-wave gate kernel waits for the
// recurrence's flags to pass a chunk, then that chunk's transposes are packed
// and its dW / dR GEMMs accumulate (beta = 1) into dw; the bias sums follow
// the recurrence.  `dw` must be zeroed on `side` before.  done = launched.
struct RnnWgradStream {
  hipStream_t side = nullptr;
  int chunks = 4;
  const float *x = nullptr;  // the layer input
  float *dw = nullptr;       // gradient (cuDNN layout)
  int max_blocks = 0;
  float in_bound = 0.f;
  bool done = false;
};
bool rnn_wgrad_stream_ok(const RnnDesc &d, int T, int N);
int rnn_backward_data(const RnnDesc &d, hipStream_t s, int T, int N, const float *y,
                      const float *dy, const float *w, float *dx, void *workspace,
                      size_t ws_bytes, void *reserve, size_t res_bytes, unsigned *err,
                      hipStream_t overlap = nullptr,  // overlap: stream for the streamed dx GEMM
                      RnnWgradStream *wgrad = nullptr,
                      const RnnPrepack *pre = nullptr);  // W^T packed by the forward (done)
struct RnnWgradOpts {
  int max_blocks = 0;             // > 0: persistent weight GEMMs of at most this many blocks
  float in_bound = 0.f;           // > 0: |x| <= in_bound (an LSTM/GRU below)
  hipStream_t s2 = nullptr;       // second stream: dW beside dR (nothing else to overlap)
  const void *in_cols = nullptr;  // bf16: x packed as columns (rnn_packed_output)
  // runs beside another component's backward recurrence (the side stream): dW
  // and dR as one launch, kept off the XCDs pinned recurrences run on
  bool beside = false;
  const RnnPrepack *pre = nullptr;  // wdone: x^T / y^T packed by the forward
};
int rnn_backward_weights(const RnnDesc &d, hipStream_t s, int T, int N, const float *x,
                         const float *y, void *workspace, size_t ws_bytes, float *dw,
                         void *reserve, size_t res_bytes, const RnnWgradOpts &o = {});

}  // namespace kctc
