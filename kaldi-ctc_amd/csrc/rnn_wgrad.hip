// rnn_wgrad.hip -- the RNN host's weight gradients (map of the units:
// rnn.hip): rnn_backward_weights (accumulates into dw, like
// cudnnRNNBackwardWeights), and the per-chunk products and bias sums of the
// weight-gradient stream (rnn_stream.hip launch_wgrad_stream).
#include "rnn_host.h"
#include "seq_align.h"

namespace kctc {
namespace {

// the dynamic tile counter of a weight GEMM (flag word kTileWordW / kTileWordR
// of the workspace: the recurrences of this layer, which use the flag area,
// are done); none without a persistent grid
int *tile_counter(const RnnWs &ws, int word, int max_blocks) {
  return max_blocks > 0 ? reinterpret_cast<int *>(ws.flags() + word) : nullptr;
}

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
  bool one_dir = false;   // dwl is one direction's block, the operands one direction's (wgrad_frames)
  long TN() const { return (long)T * N; }
  long G4() const { return (long)d.nw() * d.H; }
};

// The packed product dW (r false: A = dGates^T [dirs][G4], B = input^T, shared
// by the directions) or dR (r: A = E^T, B = shifted output^T [dirs][H]) of a
// layer over KB k blocks of frames: a batch over the directions into the
// layer's gradient block, split along K into the first split slab
X3PArgs wgrad_product(const WgradLayer &g, int KB, bool bf, bool r, const _Float16 *A, const int *eA,
                      const _Float16 *B, const int *eB) {
  const int G4 = (int)g.G4(), n = r ? g.d.H : g.d.din(g.l);
  X3PArgs x = packed_product(bf, G4, n, KB, A, eA, B, eB, g.dwl + (r ? g.roff : 0), n);
  x.beta = 1.f;
  x.batch = g.one_dir ? 1 : g.d.dirs;
  if (!g.one_dir) {
    x.sA = (long)G4 * KB * 64; x.seA = bf ? 0 : G4; x.sC = g.pls;
    if (r) { x.sB = (long)n * KB * 64; x.seB = bf ? 0 : n; }
  }
  x.split_k = x3p_pick_split(G4, n, KB, x.batch);
  x.ws = g.ws.split_slab();
  x.max_blocks = g.max_blocks;
  x.tile_counter = tile_counter(g.ws, r ? kTileWordR : kTileWordW, g.max_blocks);
  return x;
}
}  // namespace

// dW_dir += DX_dir^T x and dR_dir += DX_dir^T h_prev over the frames [ta, tb)
// of direction dir (layer 0 of a one-layer component, split-fp16, LSTM: E == DX)
void wgrad_frames(const RnnDesc &d, hipStream_t s, int T, int N, const float *x, const float *y, const RnnWs &ws,
                  float *dw, void *reserve, int max_blocks, float in_bound, int dir, int ta, int tb) {
  if (tb <= ta) return;
  const RnnReserveLayout lay = rnn_reserve_layout(d, T, N);
  const int H = d.H, dirs = d.dirs, G4 = d.nw() * H, Din = d.din(0);
  const long ldg = (long)dirs * G4, ldy = (long)dirs * H;
  const int R = (tb - ta) * N, KB = (R + 31) / 32;
  float *DX = static_cast<float *>(reserve) + lay.E;
  _Float16 *DXt = ws.at<_Float16>(ws.lay.a), *Xt = ws.at<_Float16>(ws.lay.b), *Yt = ws.at<_Float16>(ws.lay.c);
  int *eDX = ws.at<int>(ws.lay.ea), *eX = ws.at<int>(ws.lay.eb), *eY = ws.at<int>(ws.lay.ec);
  unsigned *cm = ws.at<unsigned>(ws.lay.cm);
  {
    ProfSpan ps(s, "x3_pack_w");
    pack_cols(false, s, DX + (long)ta * N * ldg + (long)dir * G4, ldg, R, G4, 0, DXt, eDX, cm, 0.f);
    pack_cols(false, s, x + (long)ta * N * Din, Din, R, Din, 0, Xt, eX, cm + G4, in_bound);
    // h_prev: direction 0 pairs frame t with y(t - 1), direction 1 with y(t + 1):
    // the rows one frame before / after the chunk's, or, where the chunk
    // meets that end of the sequence, its own rows shifted: frames outside
    // contribute zero (pack_cols zero-fills k - shift outside [0, R)).
    // (first source row, shift):  dir 0, ta == 0: (0, N)       dir 0, ta > 0: (ta - 1, 0)
    //                             dir 1, tb == T: (ta, -N)     dir 1, tb < T: (ta + 1, 0)
    const int step = dir == 0 ? -1 : 1;
    const bool edge = dir == 0 ? ta == 0 : tb == T;
    x3p_pack_cols(s, y + (long)dir * H + (long)(edge ? ta : ta + step) * N * ldy, ldy, R, H, edge ? -step * N : 0, Yt,
                  eY, nullptr, 1.f);
  }
  const LayerW lw = layer_w(d, 0);
  const WgradLayer g{d, ws, s, T, N, 0, x, y, DX, DX, dw + lw.pl0 + dir * lw.pls, lw.pls, lw.roff, max_blocks, true};
  for (int r = 0; r < 2; r++) {
    X3PArgs a = wgrad_product(g, KB, false, r, DXt, eDX, r ? Yt : Xt, r ? eY : eX);
    // (a chunk's k blocks may ask for a wider split than the slab, sized for all frames, holds)
    while (a.split_k > 1 && (long)a.split_k * G4 * a.N > ws.split_floats) a.split_k--;
    ProfSpan ps(s, r ? "gemm_bwd_r" : "gemm_bwd_w");
    gemm_x3p(s, a);
  }
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

bool rnn_wgrad_stream_ok(const RnnDesc &d, int T, int N) {
  return wgrad_stream_shape(d, T, N) && wgrad_stream_ok(plan_rec(d, N, false), d, T, N);
}

namespace {
// bf16 weight GEMMs: the transposes packed along the frames as bf16
void wgrad_bf16(const WgradLayer &g, float *R0, const RnnReserveLayout &lay, const void *in_cols) {
  const RnnDesc &d = g.d;
  const RnnWs &ws = g.ws;
  hipStream_t s = g.s;
  const int dirs = d.dirs, Din = d.din(g.l);
  const long TN = g.TN(), G4 = g.G4(), ldg = dirs * G4;
  const int KB = kblocks(true, TN);
  // the dGates transposes: written packed by the backward recurrence (bf16_direct)
  const bool pkd = bf16_direct(d, 6);
  // bf16_io: the forward wrote y^T packed (unshifted) and the backward
  // E^T shifted by one step; the input's columns may come packed from the
  // previous component's forward (in_cols)
  const bool io = bf16_io(d);
  const bool cols_in = g.l == 0 && in_cols != nullptr;
  // (bf16 halves, addressed as the packed GEMM's 2-byte operands)
  _Float16 *DXt = pkd ? reinterpret_cast<_Float16 *>(R0 + lay.pkxt) : ws.at<_Float16>(ws.lay.a);
  _Float16 *Xt = cols_in ? static_cast<_Float16 *>(const_cast<void *>(in_cols)) : ws.at<_Float16>(ws.lay.b);
  _Float16 *Yt = io ? reinterpret_cast<_Float16 *>(R0 + lay.pkyc) : ws.at<_Float16>(ws.lay.c);
  _Float16 *Et = (d.mode == kGru || io)
                     ? (pkd ? reinterpret_cast<_Float16 *>(R0 + lay.pket) : DXt + (long)dirs * G4 * KB * 64)
                     : DXt;
  {
    ProfSpan ps(s, "x3_pack_w");
    if (!pkd) {
      pack_cols(true, s, g.DX, ldg, (int)TN, (int)(dirs * G4), 0, DXt, nullptr, nullptr, 0.f);
      if (d.mode == kGru) pack_cols(true, s, g.E, ldg, (int)TN, (int)(dirs * G4), 0, Et, nullptr, nullptr, 0.f);
    }
    if (!cols_in) pack_cols(true, s, g.in, Din, (int)TN, Din, 0, Xt, nullptr, nullptr, 0.f);
    if (g.T > 1 && !io) pack_shifted_y(true, s, g.out, dirs, d.H, TN, g.N, Yt, nullptr, nullptr);
  }
  {
    ProfSpan ps(s, "gemm_bwd_w");
    gemm_x3p(s, wgrad_product(g, KB, true, false, DXt, nullptr, Xt, nullptr));
  }
  if (g.T > 1) {
    ProfSpan ps(s, "gemm_bwd_r");
    gemm_x3p(s, wgrad_product(g, KB, true, true, Et, nullptr, Yt, nullptr));
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
  const int dirs = d.dirs, Din = d.din(g.l);
  const long TN = g.TN(), G4 = g.G4();
  ProfSpan ps(s, "x3_pack_w");
  x3p_pack_cols(s, g.DX, dirs * G4, (int)TN, (int)(dirs * G4), 0, c.DXt, c.eDX, c.cme, 0.f);
  KCTC_HIP_CHECK(hipEventRecord(ev_dx, s));
  // absmax scratch of its own: the GRU-only E^T exponent array (free for an LSTM)
  unsigned *cmx = reinterpret_cast<unsigned *>(g.ws.at<int>(g.ws.lay.ed));
  if (!c.wpre) {
    pack_cols(false, s2, g.in, Din, (int)TN, Din, 0, c.Xt, c.eX, cmx, g.l == 0 ? in_bound : 0.f);
    pack_shifted_y(false, s2, g.out, dirs, d.H, TN, g.N, c.Yt, c.eY, nullptr);
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
  const int dirs = d.dirs, Din = d.din(g.l), l = g.l;
  const long TN = g.TN(), G4 = g.G4(), ldg = dirs * G4, ldy = (long)dirs * d.H;
  unsigned *cm = ws.at<unsigned>(ws.lay.cm);
  ProfSpan ps(s, "x3_pack_w");
  // (x3p_pack_cols avoid) their item counters: flag words kPackWord.. (this
  // component's recurrences, which use the flag words, are done)
  // (not beside: no word, and x3p_pack_cols then ignores the counters set below)
  PackAvoid av = beside ? avoid_pair() : PackAvoid{};
  av.counter = reinterpret_cast<int *>(ws.flags() + kPackWord);
  if (av.word) KCTC_HIP_CHECK(hipMemsetAsync(av.counter, 0, sizeof(int) * kPackWords, s));
  if (!c.cme) absmax_f32(s, g.DX, ldg, (int)TN, (int)(dirs * G4), nullptr, cm);
  x3p_pack_cols(s, g.DX, ldg, (int)TN, (int)(dirs * G4), 0, c.DXt, c.eDX, c.cme ? c.cme : cm, 0.f, av);
  if (d.mode == kGru) {
    if (!c.cme) absmax_f32(s, g.E, ldg, (int)TN, (int)(dirs * G4), nullptr, cm);
    x3p_pack_cols(s, g.E, ldg, (int)TN, (int)(dirs * G4), 0, c.Et, c.eE, c.cme ? c.cme + dirs * G4 : cm, 0.f,
                  av.at(1));
  }
  if (c.wpre) return;
  const float xb = l > 0 ? (bounded_out(d) ? 1.f : 0.f) : in_bound;
  pack_cols(false, s, g.in, Din, (int)TN, Din, 0, c.Xt, c.eX, cm, xb, av.at(2));
  if (g.T > 1) {
    if (!bounded_out(d)) absmax_f32(s, g.out, ldy, (int)TN, (int)ldy, nullptr, cm);
    pack_shifted_y(false, s, g.out, dirs, d.H, TN, g.N, c.Yt, c.eY, bounded_out(d) ? nullptr : cm, av.at(3));
  }
}

// split-fp16 weight GEMMs on operands packed over the frames (all frames: the
// shifted-out ones are zero in the packed output^T).  v6b: the layer's
// backward ran v6.
void wgrad_x3(const WgradLayer &g, bool v6b, const RnnWgradOpts &o) {
  const RnnDesc &d = g.d;
  const RnnWs &ws = g.ws;
  const PackLay &pl = ws.lay;
  hipStream_t s = g.s, s2 = o.s2;
  const RnnPrepack *pre = o.pre;
  const int H = d.H, dirs = d.dirs, Din = d.din(g.l), T = g.T;
  const long TN = g.TN(), G4 = g.G4();
  const int KBt = kblocks(false, TN);
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
    pack_wgrad_two(g, c, o.in_bound, s2, ev_dx, ev_y);
  } else {
    pack_wgrad_one(g, c, o.in_bound, o.beside);
  }
  // beside another component's pinned backward recurrence: dW and dR as
  // one launch on the CUs it leaves (gemm_x3p_pair; configs[1]: the side
  // stream fell one GEMM per layer behind, 4 ms of weight GEMMs after the
  // last recurrence)
  const bool pair = o.beside && !two && T > 1 && x3p_use_256((int)G4, Din) && x3p_use_256((int)G4, H) &&
                    g.max_blocks > 0;
  X3PArgs xw = wgrad_product(g, KBt, false, false, c.DXt, c.eDX, c.Xt, c.eX);
  // concurrent with dR: its own split slab past dR's (none when dR is not
  // split: the slabs reserve room for dR only for a split > 1)
  const long sR = x3p_pick_split((int)G4, H, KBt, dirs);
  if ((two || pair) && sR > 1) xw.ws = ws.split_slab() + (sR * dirs * G4 * H + 63) / 64 * 64;
  if (pair) {
    const PackAvoid av = avoid_pair();
    xw.max_blocks = 192;
    xw.avoid_word = av.word;
    xw.avoid_xcds = av.nxcd;
  } else {
    ProfSpan ps(sx, "gemm_bwd_w");
    gemm_x3p(sx, xw);
  }
  if (T > 1) {
    ProfSpan ps(s, "gemm_bwd_r");
    const X3PArgs x = wgrad_product(g, KBt, false, true, c.Et, c.eE, c.Yt, c.eY);
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
                         void *reserve, size_t res_bytes, const RnnWgradOpts &o) {
  // (no range check here, and a shape without a plan is not rejected)
  RnnCall c(d, T, N, workspace);
  if (!c.reserve_fits(res_bytes) || !c.workspace_fits(ws_bytes)) return KRNN_BAD_PARAM;
  c.plan(false);  // the backward recurrence that left dGates and bias partials (none: c.pl.ver 0, as before)
  const RnnReserveLayout &lay = c.lay;
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
    const WgradLayer g{d, c.ws, s, T, N, l,
                       l == 0 ? x : res + lay.per_layer * (l - 1) + lay.out,
                       (l == d.layers - 1) ? y : R0 + lay.out,
                       E, d.mode == kGru ? R0 + lay.DX : E,
                       dw + lw.pl0, lw.pls, lw.roff, o.max_blocks};
    if (x3 && d.prec == kPrecBf16) wgrad_bf16(g, R0, lay, o.in_cols);
    else if (x3) wgrad_x3(g, c.pl.ver == 6, o);
    else wgrad_f32(g);
    wgrad_bias(c.pl, d, s, T, N, dw, reserve, l);
  }
  return KRNN_OK;
}

// Length-aware: the plain pass on the un-shifted images -- the dGates that
// rnn_backward_data_seq shifted back, the caller's y and the reserve's copy of
// x, all zero on padding rows -- without the forward's prepacks or packed input
int rnn_backward_weights_seq(const RnnDesc &d, hipStream_t s, int T, int N, const int *seq_lengths, const float *x,
                             const float *y, void *workspace, size_t ws_bytes, float *dw, void *reserve,
                             size_t res_bytes, const RnnWgradOpts &o) {
  (void)x;  // its masked copy is read instead: the caller's padding rows may hold anything
  SeqLens lens;
  if (int st = seq_train_entry(d, T, N, seq_lengths, ws_bytes, res_bytes, &lens)) return st;
  const SeqTrainLay sl(d, T, N);
  RnnWgradOpts po = o;
  po.in_cols = nullptr; po.pre = nullptr;
  return rnn_backward_weights(d, s, T, N, reinterpret_cast<const float *>(static_cast<char *>(reserve) + sl.xz), y,
                              workspace, sl.ws0, dw, reserve, sl.res0, po);
}

}  // namespace kctc
