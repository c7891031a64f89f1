// rnn_stream.hip -- the RNN host's GEMMs streamed off a running v6 recurrence
// (map of the units: rnn.hip): what may stream, and the launches -- the next
// component's projection off the forward's step images or y rows, the dx GEMM
// and the chunked weight gradients off the backward's dGates rows.
#include "rnn_host.h"

namespace kctc {

// The epoch lines a stream consumer polls for the launched recurrence `p`:
// its workgroups' flag lines (flag6), or, XCD-pinned -- the flags then stay
// in the XCD's L2 -- the sc1 copies of its epochs (agg_flag6)
static const unsigned *epoch_lines(const RecLive &p) {
  return p.flags + kFlag6Word + (p.xpd ? kAggLine * kFlagStride : 0);
}

// XCDs whose every CU an XCD-pinned recurrence holds: a streamed GEMM's
// blocks landing there leave at once (xcd_word / xcd_count), and the launch
// has 8 / (8 - pinned) times the blocks so that its budget stays.  0 when the
// recurrence is not pinned or its slots take half an XCD each (configs[2]:
// all eight XCDs, 16 of each XCD's CUs left to the stream: there its blocks
// stay, on the CUs the recurrence leaves).
static int whole_pinned_xcds(const RecLive &p) {
  const int n = p.xpd && p.nwg == kCusPerXcd ? p.dirs * p.rg : 0;
  return n < 8 ? n : 0;
}

// The producer side of a streamed launch beside the recurrence `p`, for a
// budget of `budget` persistent blocks
static StreamProducer stream_producer(const RecLive &p, int budget) {
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

static bool chain_buffers_ok(const RnnFwdChain *c, int T, int N) {
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
void launch_chain_proj(const RnnDesc &d, const RecLive &p, hipEvent_t fork, int T, int N, RnnFwdChain &c,
                       unsigned *err) {
  go_beside(c.side, fork);
  const RnnDesc &n = *c.d;
  const bool bf = n.prec == kPrecBf16;
  const float *wl = c.w + n.lin_offset(0, 0, false);
  const RnnWs ws(n, T, N, c.workspace);
  X3PArgs x;
  {
    ProfSpan ps(c.side, "x3_pack_chain");
    x = proj_product(n, ws, c.side, (long)T * N, 0, wl, n.D / (bf ? 64 : 32),
                     static_cast<float *>(c.reserve) + rnn_reserve_layout(n, T, N).G);
  }
  x.A = reinterpret_cast<const _Float16 *>(p.xch); x.eA0 = bf ? 0 : 14;  // x3 images hold h 2^14
  x.tile_counter = reinterpret_cast<int *>(ws.flags());
  // every producer workgroup needs a CU of its own (96 KB LDS); the GEMM's
  // persistent blocks (96 KB each) take the rest minus a margin (chain_ok
  // checked that at least 8 fit).  No gradient exchange runs during a
  // forward pass: the updates of the previous step waited for it.
  // XCD-pinned producer: the sc1 copies of its epochs, no block on its XCDs
  x.producer = stream_producer(p, stream_block_budget(d.dirs * p.nwg * p.rg, false));
  x.stream_T = T; x.stream_N = N;
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
void launch_chain_rows(const RnnDesc &d, const RecLive &p, hipEvent_t fork, int T, int N, RnnFwdChain &c,
                       unsigned *err) {
  go_beside(c.side, fork);
  const RnnDesc &n = *c.d;
  const int NW = n.nw(), G = NW * n.H, H = d.H, KBh = H / 32, Din = n.D;
  const long TN = (long)T * N;
  const LayerW lw = layer_w(n, 0);
  const float *wl = c.w + lw.pl0;
  const RnnWs ws(n, T, N, c.workspace);
  _Float16 *Bp = ws.at<_Float16>(ws.lay.b);
  int *eB = ws.at<int>(ws.lay.eb);
  const long sB = (long)n.dirs * G * KBh * 64;
  {
    ProfSpan ps(c.side, "x3_pack_chain");
    for (int h = 0; h < 2; h++)  // K half h of the rows of both consumer directions
      x3p_pack_rows(c.side, wl + h * H, Din, G, H, Bp + h * sB, eB + h * n.dirs * G, 0.f, n.dirs, lw.pls,
                    (long)G * KBh * 64, G);
  }
  X3PBwdStream a;
  a.forward = true;
  a.M = (int)TN; a.N = n.dirs * G; a.KB = KBh;
  a.E = p.y; a.lde = 2L * H; a.edoff = H;
  a.Ap = ws.at<_Float16>(ws.lay.a); a.eA = ws.at<int>(ws.lay.ea);
  a.B = Bp; a.eB = eB; a.sB = sB; a.seB = n.dirs * G;
  a.C = static_cast<float *>(c.reserve) + rnn_reserve_layout(n, T, N).G; a.ldc = (long)n.dirs * G;
  a.bias = wl + lw.bW;
  a.bias2 = n.mode == kGru ? nullptr : wl + lw.bR;
  a.bias_cols = G; a.sbias = lw.pls;
  a.part = ws.at<float>(ws.lay.fpart);
  a.part2 = ws.at<float>(ws.lay.part2);
  a.cnt = ws.at<int>(ws.lay.cnt);
  // 128: every CU the recurrence leaves (configs[1]: 96 -> 128 blocks 720k -> 751k frames/s)
  a.producer = stream_producer(p, std::min(128, stream_block_budget(d.dirs * p.nwg * p.rg, false)));
  a.T = T; a.Nf = N; a.err = err; a.rg = p.rg;
  {
    ProfSpan ps(c.side, "fwd_proj_rows");
    gemm_x3p_bwd_stream(c.side, a);
  }
  c.done = true;
}

// W^T of layer l's dx GEMM (B operand of the streamed GEMM) into the
// workspace slot wt (per-column exponents ewt, absmax scratch cmw per direction)
void pack_dx_weights(const RnnDesc &d, int l, const float *w, const RnnWs &ws, hipStream_t st) {
  const int G4 = d.nw() * d.H, KB = G4 / (d.prec == kPrecBf16 ? 64 : 32);
  ProfSpan ps(st, "x3_pack_bwd_stream");
  pack_dx_wt(d, st, l, w + d.lin_offset(l * d.dirs, 0, false), KB, ws.at<_Float16>(ws.lay.wt), ws.at<int>(ws.lay.ewt),
             ws.at<unsigned>(ws.lay.cmw), d.din(l));
}

// dx of stacked layer l on `ov`, streamed off the backward recurrence `p`
// just launched (gemm_x3p_bwd_stream): W_d^T packed first (unless the forward
// did), then one persistent launch that packs dGates rows as the recurrence
// flags them.
void launch_bwd_stream(const RnnDesc &d, const RecLive &p, int l, const float *w, float *dxl, const RnnWs &ws,
                       int T, int N, hipStream_t ov, hipEvent_t fork, unsigned *err, const RnnPrepack *pre) {
  // (with W^T packed by the forward the GEMM starts together with the recurrence)
  go_beside(ov, fork);
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
  a.producer = stream_producer(p, std::min(t256 ? 64 : 128, stream_block_budget(d.dirs * p.nwg * p.rg, true)));
  a.T = T; a.Nf = N; a.err = err; a.rg = p.rg;
  ProfSpan ps(ov, "bwd_data_stream");
  gemm_x3p_bwd_stream(ov, a);
}

// ---------------------------------------------------------------------------
// streamed weight gradients of the bottom component (rnn.h RnnWgradStream)
// ---------------------------------------------------------------------------
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
void launch_wgrad_stream(const RecPlan &pl, const RnnDesc &d, const RecLive &p, hipEvent_t fork, int T, int N,
                         const float *y, const RnnWs &ws, void *reserve, unsigned *err, RnnWgradStream &wgrad,
                         hipStream_t s) {
  // chunk c of C: direction 0 frames [T - b(c+1), T - b(c)), direction 1
  // [b(c), b(c+1)), b(c) = c T / C; complete once every flag line holds
  // epoch b(c+1) + 2 (rows of step k are out at epoch k + 3)
  hipStream_t ws2 = wgrad.side;
  go_beside(ws2, fork);
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

}  // namespace kctc
