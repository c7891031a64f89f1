// rnn_bwd_data.hip -- the RNN host's backward-data pass (map of the units:
// rnn.hip): rnn_backward_data, dGates into the reserve and dx.
#include "rnn_host.h"
#include "seq_align.h"

namespace kctc {
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
  if (use_x3((int)G4)) {
    // dGates rows (frames, per direction) and W^T rows (input dims: columns
    // of W), packed over the gates; the absmax scratch is reused per direction
    const bool bf = d.prec == kPrecBf16, rows_in = bf && dxr;
    const int KB = kblocks(bf, G4);
    _Float16 *Ap = rows_in ? reinterpret_cast<_Float16 *>(dxr) : ws.at<_Float16>(ws.lay.a);
    _Float16 *Bp = ws.at<_Float16>(ws.lay.b);
    int *eA = ws.at<int>(ws.lay.ea), *eB = ws.at<int>(ws.lay.eb);
    {
      ProfSpan ps(s, "x3_pack");
      if (!rows_in) pack_rows(bf, s, DX, (long)dirs * G4, (int)TN, (int)G4, Ap, eA, 0.f, dirs, G4, TN * KB * 64, TN);
      pack_dx_wt(d, s, l, wl, KB, Bp, eB, ws.at<unsigned>(ws.lay.cm), 0);
    }
    for (int dir = 0; dir < dirs; dir++) {
      ProfSpan ps(s, "gemm_bwd_data");
      X3PArgs x = packed_product(bf, (int)TN, Din, KB, Ap + (long)dir * TN * KB * 64, eA + (long)dir * TN,
                                 Bp + (long)dir * Din * KB * 64, eB + dir * Din, dxl, Din);
      x.beta = dir == 0 ? 0.f : 1.f;
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
// Length-aware (rnn_backward_data_seq): the lengths and where the shifted
// images lie -- ysh (+ l * ysh_layer): layer l's output as the forward
// recurrence wrote it; dya: dy aligned; es / xs: E / DX (a GRU's) as the
// backward recurrence writes them
struct SeqBwd {
  SeqLens lens;
  const float *ysh;
  long ysh_layer;
  float *dya, *es, *xs;
};

// The layers of a backward-data pass; seq null: rnn_backward_data's
int backward_layers(const RnnDesc &d, hipStream_t s, int T, int N, const float *y, const float *dy, const float *w,
                    float *dx, RnnCall &c, void *reserve, unsigned *err, hipStream_t overlap, RnnWgradStream *wgrad,
                    const RnnPrepack *pre, const SeqBwd *seq) {
  RecScope rec_scope;  // the side launches' residency gates (beside_recurrence)
  const RnnReserveLayout &lay = c.lay; const RnnWs &ws = c.ws; const RecPlan &pl = c.pl;
  const bool v6 = pl.ver == 6;
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
    if (seq) {  // h and c in the shifted frame; dy aligned to it
      out = seq->ysh + seq->ysh_layer * l;
      seq_align_dy(s, dcur, seq->dya, T, N, d.dirs * d.H, d.H, seq->lens);
      dcur = seq->dya;
    }
    float *Er = seq ? seq->es : E, *DXr = seq ? (d.mode == kGru ? seq->xs : seq->es) : DX;
    RecParams p = rec_params(d, pl, ws, T, N, wl, lw, R0, lay, const_cast<float *>(out), err, s);
    // dx_l = sum_dir DX_dir W_dir   (lower layer's dy, or the caller's dx)
    float *dxl = (l == 0) ? dx : res + lay.per_layer * (l - 1) + lay.dout;
    // streamed: computed on `overlap` while the recurrence runs, from its rows as they appear
    const bool streamed = !seq && dxl && overlap && v6 && bwd_dx_stream_ok(pl, d, l, T, N);
    // weight gradients streamed off this recurrence (the bottom component):
    // its dGates rows must be written through too
    const bool wstream = !seq && wgrad && wgrad->side && !dxl && v6 && !p.xpd && d.layers == 1 &&
                         wgrad_stream_shape(d, T, N) && wgrad_stream_ok(pl, d, T, N);
    bwd_rec_params(p, d, pl, ws, R0, lay, dcur, Er, DXr, streamed || wstream, s);
    const hipEvent_t fork = (streamed || wstream) ? fork_event(s) : nullptr;
    RegWord &rw = reg_of_device();
    if (v6) p.reg = rw.word;  // registration for the exchange's residency gate
    RecTrace tr;
    launch_planned(d, pl, false, p, tr, rec_scope, s);
    // counted once the launch is enqueued (a failed launch never raises the target)
    if (v6) rw.expected += (unsigned long long)pl.wgs;
    g_last_bwd_scratch_free = v6 ? pl.scratch_free : true;
    if (streamed) {
      launch_bwd_stream(d, live(p), l, w, dxl, ws, T, N, overlap, fork, err, d.layers == 1 ? pre : nullptr);
      join_stream(s, overlap);
    }
    if (wstream) launch_wgrad_stream(pl, d, live(p), fork, T, N, y, ws, reserve, err, *wgrad, s);
    if (v6) xch_release(s);
    tr.dump("bwd", s, pl.grid, p.nwg, T, d.dirs, pl.ver, p.xpd);
    // the dGates images back into the un-shifted frame, padding rows +0 (the
    // recurrence leaves denormals there when its hand-off tags the payload
    // words): what the dx GEMM here and the weight GEMMs later read
    if (seq) seq_unalign_dgates(s, Er, E, DXr, DX, T, N, d.dirs * d.nw() * d.H, d.nw() * d.H, seq->lens);
    if (dxl && !streamed) dx_gemm(d, ws, s, TN, l, DX, p.dxr, wl, lw.pls, dxl);
    dcur = dxl;
  }
  return KRNN_OK;
}
}  // namespace

int rnn_backward_data(const RnnDesc &d, hipStream_t s, int T, int N, const float *y,
                      const float *dy, const float *w, float *dx, void *workspace,
                      size_t ws_bytes, void *reserve, size_t res_bytes, unsigned *err,
                      hipStream_t overlap, RnnWgradStream *wgrad, const RnnPrepack *pre) {
  if (wgrad) wgrad->done = false;
  if (!range_ok(d, T, N)) return KRNN_NOT_SUPPORTED;
  RnnCall c(d, T, N, workspace);
  if (!c.reserve_fits(res_bytes)) return KRNN_BAD_PARAM;
  if (!c.plan(false)) return KRNN_NOT_SUPPORTED;  // (before the workspace check, unlike the forward)
  if (!c.workspace_fits(ws_bytes)) return KRNN_BAD_PARAM;
  return backward_layers(d, s, T, N, y, dy, w, dx, c, reserve, err, overlap, wgrad, pre, nullptr);
}

int rnn_backward_data_seq(const RnnDesc &d, hipStream_t s, int T, int N, const int *seq_lengths, const float *y,
                          const float *dy, const float *w, float *dx, void *workspace, size_t ws_bytes,
                          void *reserve, size_t res_bytes, unsigned *err) {
  SeqBwd q;
  if (int st = seq_train_entry(d, T, N, seq_lengths, ws_bytes, res_bytes, &q.lens)) return st;
  RnnCall c(d, T, N, workspace);
  if (!c.plan(false)) return KRNN_NOT_SUPPORTED;
  const SeqTrainLay sl(d, T, N);
  char *wb = static_cast<char *>(workspace), *rb = static_cast<char *>(reserve);
  q.ysh = reinterpret_cast<const float *>(rb + sl.ysh);
  q.ysh_layer = (long)(sl.ysh_layer / sizeof(float));
  q.dya = reinterpret_cast<float *>(wb + sl.dy);
  q.es = reinterpret_cast<float *>(wb + sl.g);
  q.xs = reinterpret_cast<float *>(wb + sl.g2);
  return backward_layers(d, s, T, N, y, dy, w, dx, c, reserve, err, nullptr, nullptr, nullptr, &q);
}

}  // namespace kctc
