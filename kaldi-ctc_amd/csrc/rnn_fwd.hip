// rnn_fwd.hip -- the RNN host's forward passes (map of the units: rnn.hip):
// rnn_forward_training and the length-aware rnn_forward_inference_seq /
// rnn_forward_training_seq.
#include "rnn_host.h"
#include "seq_align.h"

namespace kctc {
namespace {

// G = in W^T + bW (+ bR) of one stacked layer, both directions, on s: packed
// bf16, packed split-fp16, or (a contraction too short to pack) fp32
void project_input(const RnnDesc &d, const RnnWs &ws, hipStream_t s, long TN, int l, const float *in,
                   const void *in_rows, const float *wl, const LayerW &lw, float *G) {
  const int NW = d.nw(), H = d.H, dirs = d.dirs, Din = d.din(l);
  if (use_x3(Din, 32)) {
    // input rows and W rows packed: bf16 (the rows may come packed from the
    // previous component's forward, in_rows) or split-fp16 (a lower stacked
    // layer's output is bounded; the component input and RELU outputs get
    // per-row exponents); fp32 accumulation
    const bool bf = d.prec == kPrecBf16, rows_in = bf && l == 0 && in_rows && Din % 64 == 0;
    _Float16 *Ap = rows_in ? static_cast<_Float16 *>(const_cast<void *>(in_rows)) : ws.at<_Float16>(ws.lay.a);
    int *eA = ws.at<int>(ws.lay.ea);
    X3PArgs x;
    {
      ProfSpan ps(s, "x3_pack");
      if (!rows_in) pack_rows(bf, s, in, Din, (int)TN, Din, Ap, eA, (l > 0 && bounded_out(d)) ? 1.f : 0.f);
      x = proj_product(d, ws, s, TN, l, wl, kblocks(bf, Din), G);
    }
    x.A = Ap;
    if (!bf) x.eA = eA;
    ProfSpan ps(s, "gemm_fwd_proj");
    gemm_x3p(s, x);
  } else {
    GemmArgs g;
    g.transA = false; g.transB = true;
    g.M = (int)TN; g.N = NW * H; g.K = Din;
    g.A = in; g.lda = Din;
    g.B = wl; g.ldb = Din;
    g.C = G; g.ldc = (long)dirs * NW * H;
    g.bias = wl + lw.bW; g.bias2 = (d.mode == kGru) ? nullptr : wl + lw.bR;
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
  PackAvoid av = avoid_pair();
  av.counter = ws.at<int>(ws.lay.pcnt);  // item counters: x^T, then y^T per direction
  KCTC_HIP_CHECK(hipMemsetAsync(av.counter, 0, sizeof(int) * 3, ss));
  ProfSpan ps(ss, "x3_pack_w_fwd");
  x3p_pack_cols(ss, in, Din, (int)TN, Din, 0, ws.at<_Float16>(ws.lay.xt), ws.at<int>(ws.lay.ext), nullptr,
                pre.in_bound, av);
}
// ... and y^T after it (and after the joins: s does not wait for it)
void prepack_y_cols(const RnnDesc &d, const RnnWs &ws, const float *out, long TN, int N, RnnPrepack &pre,
                    hipStream_t s) {
  hipStream_t ss = pre.stream;
  KCTC_HIP_CHECK(hipStreamWaitEvent(ss, fork_event(s), 0));
  PackAvoid av = avoid_pair();
  av.counter = ws.at<int>(ws.lay.pcnt) + 1;
  {
    ProfSpan ps(ss, "x3_pack_w_fwd");
    pack_shifted_y(false, ss, out, d.dirs, d.H, TN, N, ws.at<_Float16>(ws.lay.yt), ws.at<int>(ws.lay.eyt), nullptr,
                   av);
  }
  KCTC_HIP_CHECK(hipEventRecord(pre.wev, ss));
  pre.wdone = true;
}

}  // namespace

int rnn_forward_training(const RnnDesc &d, hipStream_t s, int T, int N, const float *x,
                         const float *w, float *y, void *workspace, size_t ws_bytes,
                         void *reserve, size_t res_bytes, unsigned *err, const RnnFwdOpts &o) {
  RecScope rec_scope;  // the side launches' residency gates (beside_recurrence)
  RnnFwdChain *chain = o.chain; RnnPrepack *pre = o.pre;
  if (chain) chain->done = false;
  if (pre) pre->done = pre->wdone = false;
  if (!range_ok(d, T, N)) return KRNN_NOT_SUPPORTED;
  RnnCall c(d, T, N, workspace);
  if (!c.reserve_fits(res_bytes) || !c.workspace_fits(ws_bytes)) return KRNN_BAD_PARAM;
  if (!c.plan(true)) return KRNN_NOT_SUPPORTED;
  const RnnReserveLayout &lay = c.lay; const RnnWs &ws = c.ws; const RecPlan &pl = c.pl;
  const bool v6 = pl.ver == 6;
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
    if (!(l == 0 && o.input_projected)) project_input(d, ws, s, TN, l, in, o.in_rows, wl, lw, R0 + lay.G);
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
      go_beside(pre->stream, fork);
      pack_dx_weights(d, 0, w, ws, pre->stream);
      KCTC_HIP_CHECK(hipEventRecord(pre->ev, pre->stream));
      pre->done = true;
    }
    if (prepack_w) {
      go_beside(pre->stream, prepack ? nullptr : fork);  // (the dx prepack waited for the fork already)
      prepack_x_cols(d, ws, in, TN, *pre);
    }
    if (chained) {
      launch_chain_proj(d, live(p), fork, T, N, *chain, err);
      join_stream(s, chain->side);
    }
    if (rowchain) {
      launch_chain_rows(d, live(p), fork, T, N, *chain, err);
      join_stream(s, chain->side);
    }
    if (prepack_w) prepack_y_cols(d, ws, out, TN, N, *pre, s);
    tr.dump("fwd", s, pl.grid, p.nwg, T, d.dirs, pl.ver, p.xpd);
    in = out;
  }
  return KRNN_OK;
}

// ---------------------------------------------------------------------------
// length-aware inference (rnn.h rnn_forward_inference_seq)
// ---------------------------------------------------------------------------
namespace {
// the seq buffer: the layer-0 input with its padding zeroed, one layer's
// projected G before the shift, one layer's output before the shift back
struct SeqBuf {
  size_t xz = 0, g = 0, y = 0, total = 0;
  SeqBuf(const RnnDesc &d, int T, int N) {
    const size_t TN = (size_t)T * N;
    g = align_up(sizeof(float) * TN * d.D, 256);
    y = g + (d.dirs == 2 ? align_up(sizeof(float) * TN * d.dirs * d.nw() * d.H, 256) : 0);
    total = y + align_up(sizeof(float) * TN * d.dirs * d.H, 256);
  }
};
}  // namespace

size_t rnn_seq_buffer_bytes(const RnnDesc &d, int T, int N) { return SeqBuf(d, T, N).total; }

namespace {
// What the length-aware forwards share.  xz: the layer-0 input with its
// padding zeroed; gs: one layer's projected G before the shift; ys: the
// recurrence's output before the shift back -- one image reused by every
// stacked layer (ys_layer 0: inference) or one per layer, ys_layer floats
// apart, kept for the backward recurrence (training).
int forward_seq(const RnnDesc &d, hipStream_t s, int T, int N, const SeqLens &lens, bool train, const float *x,
                const float *w, float *y, RnnCall &c, void *reserve, float *xz, float *gs, float *ys, long ys_layer,
                unsigned *err) {
  RecScope rec_scope;
  const RnnReserveLayout &lay = c.lay; const RnnWs &ws = c.ws; const RecPlan &pl = c.pl;
  const int H = d.H, dirs = d.dirs, NW = d.nw();
  const long TN = (long)T * N;
  float *res = static_cast<float *>(reserve);
  // (the training passes: the same maps under profile names of their own)
  const auto align = train ? seq_align_train : seq_align;
  const auto unalign = train ? seq_unalign_train : seq_unalign;
  // padding rows of the input may hold anything: zeroed before the projection
  align(s, x, xz, T, N, d.D, d.D, lens);
  const float *in = xz;
  for (int l = 0; l < d.layers; l++) {
    const bool last = l == d.layers - 1;
    float *R0 = res + lay.per_layer * l;
    float *out = last ? y : R0 + lay.out;
    float *ysl = ys + ys_layer * l;
    const LayerW lw = layer_w(d, l);
    const float *wl = w + lw.pl0;
    // no streamed hand-over and no packed input rows here: they read
    // un-shifted images
    if (dirs == 2) {
      // the reverse direction's gate columns move right by T - len[n] frames,
      // so that every sequence ends at row T-1 where that recurrence starts
      project_input(d, ws, s, TN, l, in, nullptr, wl, lw, gs);
      align(s, gs, R0 + lay.G, T, N, dirs * NW * H, NW * H, lens);
    } else {
      project_input(d, ws, s, TN, l, in, nullptr, wl, lw, R0 + lay.G);
    }
    RecParams p = rec_params(d, pl, ws, T, N, wl, lw, R0, lay, ysl, err, s);
    fwd_rec_params(p, d, pl, ws, R0, lay, false, false, s);
    RecTrace tr;
    launch_planned(d, pl, true, p, tr, rec_scope, s);
    tr.dump("fwd", s, pl.grid, p.nwg, T, dirs, pl.ver, p.xpd);
    // ... and its output moves back; padding rows of both directions become 0
    unalign(s, ysl, out, T, N, dirs * H, H, lens);
    in = out;
  }
  return KRNN_OK;
}
}  // namespace

int rnn_forward_inference_seq(const RnnDesc &d, hipStream_t s, int T, int N, const int *seq_lengths, const float *x,
                              const float *w, float *y, void *workspace, size_t ws_bytes, void *reserve,
                              size_t res_bytes, void *seq_buffer, size_t seq_bytes, unsigned *err) {
  if (!range_ok(d, T, N)) return KRNN_NOT_SUPPORTED;
  SeqLens lens;
  if (!seq_lens(seq_lengths, T, N, &lens)) return KRNN_BAD_PARAM;
  RnnCall c(d, T, N, workspace);
  if (!c.reserve_fits(res_bytes) || !c.workspace_fits(ws_bytes)) return KRNN_BAD_PARAM;
  const SeqBuf sb(d, T, N);
  if (!seq_buffer || seq_bytes < sb.total) return KRNN_BAD_PARAM;
  if (!c.plan(true)) return KRNN_NOT_SUPPORTED;
  char *sbase = static_cast<char *>(seq_buffer);
  return forward_seq(d, s, T, N, lens, false, x, w, y, c, reserve, reinterpret_cast<float *>(sbase + sb.xz),
                     reinterpret_cast<float *>(sbase + sb.g), reinterpret_cast<float *>(sbase + sb.y), 0, err);
}

// ---------------------------------------------------------------------------
// length-aware training (rnn.h rnn_forward_training_seq)
// ---------------------------------------------------------------------------
SeqTrainLay::SeqTrainLay(const RnnDesc &d, int T, int N) {
  const size_t TN = (size_t)T * N;
  const size_t gates = align_up(sizeof(float) * TN * d.dirs * d.nw() * d.H, 256);
  const size_t outs = align_up(sizeof(float) * TN * d.dirs * d.H, 256);
  ws0 = align_up(rnn_workspace_bytes(d, T, N), 256);
  g = ws0;
  g2 = g + gates;
  dy = g2 + (d.mode == kGru ? gates : 0);
  ws_total = dy + outs;
  res0 = align_up(sizeof(float) * (size_t)rnn_reserve_layout(d, T, N).total, 256);
  xz = res0;
  ysh = xz + align_up(sizeof(float) * TN * d.D, 256);
  ysh_layer = outs;
  res_total = ysh + outs * d.layers;
}

size_t rnn_seq_train_workspace_bytes(const RnnDesc &d, int T, int N) { return SeqTrainLay(d, T, N).ws_total; }
size_t rnn_seq_train_reserve_bytes(const RnnDesc &d, int T, int N) { return SeqTrainLay(d, T, N).res_total; }

int seq_train_entry(const RnnDesc &d, int T, int N, const int *seq_lengths, size_t ws_bytes, size_t res_bytes,
                    SeqLens *lens) {
  if (!range_ok(d, T, N)) return KRNN_NOT_SUPPORTED;
  if (d.prec == kPrecBf16) return KRNN_NOT_SUPPORTED;  // its direct path leaves no fp32 dGates rows to un-shift
  if (!seq_lens(seq_lengths, T, N, lens)) return KRNN_BAD_PARAM;
  const SeqTrainLay sl(d, T, N);
  if (ws_bytes < sl.ws_total || res_bytes < sl.res_total) return KRNN_BAD_PARAM;
  return KRNN_OK;
}

int rnn_forward_training_seq(const RnnDesc &d, hipStream_t s, int T, int N, const int *seq_lengths, const float *x,
                             const float *w, float *y, void *workspace, size_t ws_bytes, void *reserve,
                             size_t res_bytes, unsigned *err) {
  SeqLens lens;
  if (int st = seq_train_entry(d, T, N, seq_lengths, ws_bytes, res_bytes, &lens)) return st;
  RnnCall c(d, T, N, workspace);
  if (!c.plan(true)) return KRNN_NOT_SUPPORTED;
  const SeqTrainLay sl(d, T, N);
  char *wb = static_cast<char *>(workspace), *rb = static_cast<char *>(reserve);
  return forward_seq(d, s, T, N, lens, true, x, w, y, c, reserve, reinterpret_cast<float *>(rb + sl.xz),
                     reinterpret_cast<float *>(wb + sl.g), reinterpret_cast<float *>(rb + sl.ysh),
                     (long)(sl.ysh_layer / sizeof(float)), err);
}

}  // namespace kctc
