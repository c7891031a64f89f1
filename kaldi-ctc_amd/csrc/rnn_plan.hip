// rnn_plan.hip -- layout and plan of the RNN host (rnn.hip): the training
// reserve and the workspace (RnnWs), and which recurrence a (descriptor, N)
// runs in each direction of time and how it is launched (plan_rec).
#include <initializer_list>
#include <map>

#include "common.h"
#include "gemm.h"
#include "gemm_x3p.h"
#include "rnn_plan.h"

namespace kctc {

static long al64(long x) { return (x + 63) / 64 * 64; }

RnnReserveLayout rnn_reserve_layout(const RnnDesc &d, int T, int N) {
  RnnReserveLayout r;
  const long TN = (long)T * N, nw = d.nw(), H = d.H, dirs = d.dirs;
  long p = 0;
  r.G = p;    p += al64(TN * dirs * nw * H);
  r.aux = p;  p += al64(TN * dirs * H);
  r.E = p;    p += al64(TN * dirs * nw * H);
  r.DX = p;   p += (d.mode == kGru) ? al64(TN * dirs * nw * H) : 0;
  r.bias = p; p += al64(dirs * 2 * nw * H * (long)((N + 7) / 8));  // v6: per row group (>= 8 rows each)
  r.out = p;  p += (d.layers > 1) ? al64(TN * dirs * H) : 0;
  r.dout = p; p += (d.layers > 1) ? al64(TN * dirs * H) : 0;
  r.kbt64 = (TN + 63) / 64 * 64;
  const bool pkd = d.prec == kPrecBf16 && d.layers == 1 && d.pk;  // bf16 halves: 2 per float
  const long G4 = nw * H, kbg64 = (G4 + 63) / 64 * 64;
  r.pkxr = p; p += pkd ? al64((dirs * TN * kbg64 + 1) / 2) : 0;
  r.pkxt = p; p += pkd ? al64((dirs * G4 * r.kbt64 + 1) / 2) : 0;
  const bool io = pkd && d.layers == 1 && dirs == 2;  // bf16_io: E^T shifted, apart from DX^T
  r.pket = p; p += (pkd && (d.mode == kGru || io)) ? al64((dirs * G4 * r.kbt64 + 1) / 2) : 0;
  r.pkyr = p; p += io ? al64((TN * dirs * H + 1) / 2) : 0;
  r.pkyc = p; p += io ? al64((dirs * H * r.kbt64 + 1) / 2) : 0;
  r.per_layer = p;
  r.total = p * d.layers;
  return r;
}

// ---------------------------------------------------------------------------
// workspace
// ---------------------------------------------------------------------------
static long drec_split_floats(const RnnDesc &d, int T, int N) {
  // the dR and dW split slabs of a layer side by side: with a second stream
  // (rnn_backward_weights' s2) the two GEMMs run concurrently
  long needR = 0, needW = 0;
  const int G4 = d.nw() * d.H;
  const int KB = (int)(((long)T * N + 31) / 32);  // packed k blocks over the frames (x3; bf16 needs fewer)
  for (int l = 0; l < d.layers; l++) {
    const long K = (long)(T > 1 ? T - 1 : 1) * N;
    int s = std::max(gemm_pick_split(G4, d.H, (int)K, d.dirs), x3p_pick_split(G4, d.H, KB, d.dirs));
    if (s > 1) needR = std::max(needR, (long)s * d.dirs * G4 * d.H);
    s = std::max(gemm_pick_split(G4, d.din(l), (int)((long)T * N), d.dirs), x3p_pick_split(G4, d.din(l), KB, d.dirs));
    if (s > 1) needW = std::max(needW, (long)s * d.dirs * G4 * d.din(l));
  }
  return al64(needR) + needW;
}
// the exchange images (one layer at a time; forward and backward of a layer
// never overlap)
static size_t xch_bytes(const RnnDesc &d, int T, int N) {
  const long Npad = (N + 15) / 16 * 16;
  // generic images: 4 B x dirs x nW x H x Npad per step; the v6 forward's
  // [2 dirs][H/32][hi, lo][16][32] halves per row group of <= 16 rows (at most
  // 2 Npad / 16 groups): 16 B x H x Npad.  + 2 steps: the v6 forward's ring of
  // hand-off images after its T step images
  const size_t per = std::max<size_t>(sizeof(float) * d.dirs * d.nw(), 16);
  return per * (size_t)(T + 2) * d.H * Npad;
}
static PackLay pack_layout(const RnnDesc &d, int T, int N) {
  const long TN = (long)T * N, G = (long)d.nw() * d.H, Dm = std::max(d.D, d.dirs * d.H), dirs = d.dirs;
  const size_t fw_a = x3p_bytes(TN, Dm), fw_b = x3p_bytes(dirs * G, Dm);
  const size_t bd_a = x3p_bytes(dirs * TN, G), bd_b = x3p_bytes(dirs * Dm, G);
  const size_t bw_a = x3p_bytes(dirs * G, TN) * (d.mode == kGru ? 2 : 1), bw_b = x3p_bytes(Dm, TN),
               bw_c = x3p_bytes(dirs * d.H, TN);
  PackLay p;
  size_t o = 0;
  p.a = o; o = align_up(o + std::max({fw_a, bd_a, bw_a}), 256);
  p.b = o; o = align_up(o + std::max({fw_b, bd_b, bw_b}), 256);
  p.c = o; o = align_up(o + bw_c, 256);
  const long ne = std::max({TN * dirs, dirs * G * 2, dirs * Dm}) + 64;
  p.ea = o; o = align_up(o + sizeof(int) * ne, 256);
  p.eb = o; o = align_up(o + sizeof(int) * ne, 256);
  p.ec = o; o = align_up(o + sizeof(int) * ne, 256);
  p.ed = o; o = align_up(o + sizeof(int) * ne, 256);
  p.cm = o; o = align_up(o + sizeof(unsigned) * ne, 256);
  p.part = o; o = align_up(o + sizeof(float) * x3p_bwd_stream_part_floats((int)TN, (int)Dm), 256);  // backward stream partials
  // (also the row stream of this component's projection off the previous
  // component's forward, launch_chain_rows: N = dirs * G columns)
  p.cnt = o; o = align_up(o + sizeof(int) * x3p_bwd_stream_ints((int)TN, (int)std::max(Dm, dirs * G)), 256);
  p.part2 = o; o = align_up(o + sizeof(float) * x3p_bwd_stream_part2_floats((int)std::max(Dm, dirs * G)), 256);
  p.cme = o; o = align_up(o + sizeof(unsigned) * 2 * dirs * G, 256);  // dGates column maxima (v6 backward)
  // arrival counters of the direction-split streamed projection (this component as its consumer)
  p.fcnt = o; o = align_up(o + sizeof(int) * ((TN + 127) / 128 * dirs * ((G + 127) / 128) + 64), 256);
  p.fpart = o; o = align_up(o + sizeof(float) * std::max((size_t)((TN + 127) / 128) * dirs * ((G + 127) / 128) * 128 * 128,
                                                          x3p_bwd_stream_part_floats((int)TN, (int)(dirs * G))), 256);
  // W^T of the streamed dx GEMM, packed by the forward (RnnPrepack): kept
  // from the forward to the backward, apart from every other slot
  p.wt = o; o = align_up(o + x3p_bytes(dirs * Dm, G), 256);
  p.ewt = o; o = align_up(o + sizeof(int) * (dirs * Dm + 64), 256);
  p.cmw = o; o = align_up(o + sizeof(unsigned) * (dirs * Dm + 64), 256);
  // x^T / y^T of the weight GEMMs, packed by the forward (RnnPrepack::wgrad)
  p.xt = o; o = align_up(o + bw_b, 256);
  p.yt = o; o = align_up(o + bw_c, 256);
  p.ext = o; o = align_up(o + sizeof(int) * (Dm + 64), 256);
  p.eyt = o; o = align_up(o + sizeof(int) * (dirs * d.H + 64), 256);
  // item counters of those packs (on the prepack stream; apart from the
  // recurrence flags, which the backward resets on the compute stream)
  p.pcnt = o; o = align_up(o + sizeof(int) * 4, 256);
  p.total = o;
  return p;
}
RnnWs::RnnWs(const RnnDesc &d, int T, int N, void *workspace)
    : lay(pack_layout(d, T, N)), split_floats(drec_split_floats(d, T, N)), base(static_cast<char *>(workspace)) {
  flags_off = sizeof(float) * (size_t)al64(split_floats);
  xch_off = flags_off + kFlagBytes;
  pack_off = align_up(xch_off + xch_bytes(d, T, N), 256);
}
size_t rnn_workspace_bytes(const RnnDesc &d, int T, int N) { return RnnWs(d, T, N, nullptr).bytes(); }

// ---------------------------------------------------------------------------
// CU budget (rnn.h)
// ---------------------------------------------------------------------------
static int g_usable_cus = 0, g_comm_cus = 0;
void rnn_set_cu_budget(int cus, int comm) {
  g_usable_cus = std::max(0, cus);
  g_comm_cus = std::max(0, comm);
}
int rnn_usable_cus() {
  static int dev_cus[64] = {0};
  int dev = 0;
  KCTC_HIP_CHECK(hipGetDevice(&dev));
  int &c = dev_cus[dev & 63];
  if (!c) KCTC_HIP_CHECK(hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev));
  return g_usable_cus > 0 ? std::min(g_usable_cus, c) : c;
}
int rnn_comm_cus() { return g_comm_cus; }

int stream_block_budget(int rec_wgs, bool backward) {
  // the 16-CU margin keeps room for the exchange's kernels beyond maxCTAs;
  // a backward without an exchange (one rank) gives the streamed dx GEMM all
  // CUs the recurrence leaves (configs[1]: 128 blocks, 655.7k -> 670.7k frames/s)
  const int margin = backward && rnn_comm_cus() == 0 ? 0 : 16;
  const int left = rnn_usable_cus() - rec_wgs - (backward ? rnn_comm_cus() : 0) - margin;
  return left >= 8 ? left : 0;
}

// ---------------------------------------------------------------------------
// which recurrence
// ---------------------------------------------------------------------------
namespace {

size_t fwd_lds_bytes(const RnnDesc &d, int N, int U) {
  const int ncol = (d.nw() * U + 15) / 16 * 16, Npad = (N + 15) / 16 * 16;
  return sizeof(float) * ((size_t)ncol * (d.H + 4) + 4 * (size_t)Npad * ncol);
}
size_t bwd_lds_bytes(const RnnDesc &d, int N, int U) {
  const int Npad = (N + 15) / 16 * 16;
  return sizeof(float) * ((size_t)U * (d.nw() * d.H + 4) + std::max(4 * (size_t)Npad * 16, (size_t)2 * N * U * d.nw()));
}

// Generic recurrences: U units per workgroup, nwg = H / U workgroups per direction.
// XCD slots one direction spans for U (slot mapping: part of one slot, or 1,
// 2, 4 or 8 whole slots of kCusPerXcd workgroups; 0: no such partition)
int slot_xpd(const RnnDesc &d, int U) {
  if (U <= 0 || d.H % U || d.dirs > 8) return 0;
  const int nwg = d.H / U;
  if (nwg % kCusPerXcd) return nwg < kCusPerXcd ? 1 : 0;
  const int x = nwg / kCusPerXcd;
  return (x == 1 || x == 2 || x == 4 || x == 8) && x * d.dirs <= 8 ? x : 0;
}
// U and RecPlan::xpd of (d, N) in one direction of time: the first U of the
// slot-mapped order that fits, else the first of the plain-mapped order (xpd
// 0, every workgroup resident: dirs * nwg <= 256 = one per CU); U 0: none fits
struct GenericU {
  int U = 0, xpd = 0;
};
GenericU pick_generic_u(const RnnDesc &d, int N, bool fwd) {
  auto fits = [&](int U) {  // the kernels' own limits
    if (d.H % U || N * U > kMaxEPT * NT) return false;
    if (fwd) return d.nw() * U <= 16 * kMaxCT && fwd_lds_bytes(d, N, U) <= 160 * 1024;
    return U <= 16 && bwd_lds_bytes(d, N, U) <= 160 * 1024;
  };
  auto first = [&](std::initializer_list<int> order, bool slots) {
    for (int U : order) {
      if (!fits(U)) continue;
      if (slots && slot_xpd(d, U)) return GenericU{U, slot_xpd(d, U)};
      if (!slots && (long)d.dirs * (d.H / U) <= 256) return GenericU{U, 0};
    }
    return GenericU{};
  };
  // forward, slot-mapped, measured on BLSTM-512 N=16 (1 x MI355X): U=8 (2 XCD
  // slots per direction) 44 ms/step of forward recurrence, U=4 48, U=16 58
  const GenericU c = fwd ? first({8, 16, 4, 32}, true) : first({16, 8, 4}, true);
  if (c.U) return c;
  // plain, forward: the smallest U that keeps every workgroup resident
  // (per-step MFMA latency falls with U)
  return fwd ? first({4, 8, 16}, false) : first({16, 8, 4}, false);
}

// v6 recurrences (LSTM / GRU): one configuration for a (shape, N):
//   rg   row groups of 16 sequences, each an independent recurrence
//   U    units per workgroup (8, 16 at 256 threads; 32 at 512 threads)
// chosen so that dirs * (H / U) * rg workgroups (one per CU, >= 96 KB LDS
// each) stay within 128 workgroups (half the chip, the rest
// for the GEMMs that overlap the recurrences).  Preference U = 16, then 32,
// then 8 (measured on BLSTM-512 N=16: U=16 34.2 ms/step of forward
// recurrence, U=8 37.1).
// Sequences per v6 row group: 16 (one MFMA row tile), or 8 for 9 <= N <= 32
// -- the batch then runs as ceil(N / 8) independent recurrences side by side,
// each moving half the hand-off rows per step.  Default 8 for N <= 16
// (configs[1]: forward 28.0 -> 27.0, backward 34.2 -> 33.0 ms/step of
// recurrence; the weight GEMMs beside the backward get 64 CUs fewer and take
// twice as long, still hidden).  KCTC_REC_GS sets both directions; a set
// knob applies up to N = 32.  pick6
// falls back to 16 when no workgroup partition fits the groups of 8.
int v6_group_rows(int N) {
  const int want = env_int("KCTC_REC_GS", N <= 16 ? 8 : 16);
  return (want == 8 && N > 8 && N <= 32) ? 8 : 16;
}
V6Cfg pick6(const RnnDesc &d, int N, bool fwd, int gs_force = 0) {
  V6Cfg c;
  if ((d.mode != kLstm && d.mode != kGru) || N <= 0 || N > 64 || d.dirs > 2) return c;
  if (d.H != 256 && d.H != 320 && d.H != 512 && d.H != 1024) return c;
  const int gs = gs_force ? gs_force : v6_group_rows(N), rg = (N + gs - 1) / gs;
  // never more workgroups than the CUs this process may use (all must be resident)
  const int max_wg = std::min(128, rnn_usable_cus());
  auto ok = [&](int U) {
    const int nth = U == 32 ? 512 : 256, nwv = nth / 64;
    if (d.H % U || d.H % (16 * nwv) || (d.H / U) % (nth / (4 * U))) return false;
    return (long)d.dirs * (d.H / U) * rg <= std::max(max_wg, d.dirs * (d.H / U));  // rg = 1 always fits
  };
  auto take = [&](int U) {
    c.U = U;
    // U = 16 at H = 512 runs 512 threads (K split over 8 waves; measured on
    // BLSTM-512 N=16: forward 31.9 -> 28.4, backward 34.4 -> 32.9 ms/step of
    // recurrence vs 256 threads; 1024 threads 30.5 / 33.5)
    c.nth = U == 32 ? 512 : (U == 16 && d.H == 512) ? 512 : 256;
    c.rg = rg;
    c.gs = gs;
    // The kernel variant, at U = 16 / 512 threads.  Row groups of <= 8
    // sequences: hi / lo stacked in one MFMA operand (all four products:
    // equally accurate or better), on by default in both directions: the
    // stacked forward (one A load per k block, 2/3 of the MFMAs) runs 1.76
    // us/step against 2.05 for the IO-wave forward (round 4); the transposed
    // stacked backward with its DPP row fold 1.91 against 2.43 (round 5).
    // KCTC_STK_FWD (forward; KCTC_STK for both).  Else the forward runs
    // with IO waves (the G loads off the hand-off waves).
    const bool wide16 = U == 16 && c.nth == 512;
    const int stk = fwd ? env_int("KCTC_STK_FWD", env_int("KCTC_STK", 1)) : env_int("KCTC_STK", 1);
    const bool stacked = wide16 && d.prec != kPrecBf16 && gs <= 8 && stk;
    c.variant = stacked ? kRec6Stacked : wide16 && fwd ? kRec6IoWave : kRec6Plain;
    return c;
  };
  for (int U : {16, 32, 8})
    if (ok(U)) {
      // rg = 1 keeps the measured N <= 16 choice even above the budget
      if (rg == 1 || (long)d.dirs * (d.H / U) * rg <= max_wg) return take(U);
    }
  return gs == 8 ? pick6(d, N, fwd, 16) : c;
}

size_t fwd6_lds_bytes(const RnnDesc &d, const V6Cfg &c) {
  const int CT = (d.nw() * c.U + 15) / 16, nwv = c.nth / 64, np = d.prec == kPrecBf16 ? 1 : 2;
  const size_t rp = std::max(CT * 16 + 1, 4 * c.U);  // rnn_fwd_rec6's RPR (float4 K partials)
  // + the IO waves' G (and output) slots; the stacked forward's launch keeps them (forward cfg only)
  const bool iow = c.variant == kRec6IoWave || c.variant == kRec6Stacked;
  const size_t b = sizeof(float) * (nwv * 16 * rp + 8) + np * 16 * (size_t)c.U * 2 + 16 +
                   (iow ? sizeof(float) * 16 * c.U * (8 * d.nw() + 2 * (d.nw() + 2)) + 16 + 4 * 64 * 4 : 0);
  return std::max(b, (size_t)96 * 1024);  // one recurrence workgroup per CU
}
size_t bwd6_lds_bytes(const RnnDesc &d, const V6Cfg &c) {
  const int K = d.nw() * c.U, KB = (K + 31) / 32, AP = KB * 32 + 8;
  const size_t img = (d.prec == kPrecBf16 ? 1 : 2) * 16 * (size_t)AP * 2;
  const size_t red = sizeof(float) * std::max((size_t)c.nth * 4, (size_t)2 * 16 * c.U * d.nw());
  // dGates tile staged for write-through, and (bf16, packed writes) the E tile beside it
  const size_t estg = sizeof(float) * 16 * c.U * d.nw() * (d.prec == kPrecBf16 ? 2 : 1);
  // at least 96 KB so that no other workgroup (a side-stream GEMM block)
  // shares the CU with a recurrence workgroup
  return std::max(img + red + estg, (size_t)96 * 1024);
}

// Does the v6 recurrence kernel `k` run without scratch (no register
// spills)?  Nothing runs beside one that does.  Round 6 first blamed scratch
// for configs[4]'s KCTC_STREAM_ALL hang (the bf16 GRU backward, then 124 B of
// spills per lane, stayed short of its 32 workgroups on one XCD for 0.4 s
// behind the one-wave residency wait of its dx stream); with the spills gone
// it hung the same way: the cause is its 256 VGPRs x 2 waves per SIMD, a
// whole CU's register file, which no workgroup gets on a CU where a gate wave
// sits -- gate_kernel's blocks now leave the recurrence's XCDs
// (tests/test_fullsize_gpu.py cfg4+stream_all).  The scratch
// condition stays as a precaution.
bool rec6_scratch_free(const void *k) {
  static thread_local std::map<const void *, bool> memo;
  auto it = memo.find(k);
  if (it != memo.end()) return it->second;
  hipFuncAttributes a{};
  KCTC_HIP_CHECK(hipFuncGetAttributes(&a, k));
  return memo[k] = a.localSizeBytes == 0;
}

// XCDs an XCD-pinned v6 recurrence occupies (bit x: XCD x), 0
// when it is not pinned: every (row group, direction) runs on one XCD, its
// H / U workgroups on kCusPerXcd (configs[1] / [4]: 32) or kCusPerXcd / 2
// (configs[2]: U = 32 at H = 512, four row groups x two directions = all
// eight XCDs, half of each XCD's CUs) of that XCD's CUs, and the whole chip's
// CUs must be usable (no CU partition).  KCTC_XCD6=0 / KCTC_XCD6F=0 switch it
// off; the 16-workgroup shapes pin too (configs[2]
// pinned: 990k -> 1.12M frames/s, forward 3.14 -> 2.42, backward 4.52 -> 3.53
// us/step, same box).
unsigned xcd_mask(const RnnDesc &d, const V6Cfg &c6, bool fwd) {
  if (!c6 || d.dirs * c6.rg > 8) return 0;
  const int nwg = d.H / c6.U;
  if (nwg != kCusPerXcd && nwg != kCusPerXcd / 2) return 0;
  if (!env_int(fwd ? "KCTC_XCD6F" : "KCTC_XCD6", 1)) return 0;
  int dev = 0, cus = 0;
  KCTC_HIP_CHECK(hipGetDevice(&dev));
  KCTC_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  if (rnn_usable_cus() != cus || cus != 8 * kCusPerXcd) return 0;
  // backward: an exchange's kernels (comm stream) landing on a pinned XCD
  // would hold the recurrence's CUs there until the all-reduce ends, and a
  // stream CU mask cannot keep them off an XCD (scripts/cumask_probe.hip:
  // each mask bit selects one CU in every XCD): pinned only without an
  // exchange.  No exchange kernel runs during a forward pass (the previous
  // step's updates waited for every bucket), so the forward stays pinned.
  // With a residency-gated exchange (rnn_set_comm_gated) no exchange kernel
  // is in flight while a backward recurrence becomes resident, so it stays pinned.
  if (!fwd && rnn_comm_cus() > 0 && !rnn_comm_gated()) return 0;
  return (1u << (d.dirs * c6.rg)) - 1u;
}

}  // namespace

RecPlan plan_rec(const RnnDesc &d, int N, bool fwd) {
  RecPlan pl;
  const V6Cfg c6 = pick6(d, N, fwd);
  const GenericU gu = c6 ? GenericU{} : pick_generic_u(d, N, fwd);
  const int U = c6 ? c6.U : gu.U;
  if (d.prec == kPrecBf16 && !c6) return pl;  // bf16 exists on v6 only
  if (!U) return pl;
  pl.ver = c6 ? 6 : 4;
  pl.U = U;
  pl.nwg = d.H / U;
  if (c6) {
    pl.c6 = c6;
    pl.nth = c6.nth;
    pl.lds = fwd ? fwd6_lds_bytes(d, c6) : bwd6_lds_bytes(d, c6);
    pl.rg = c6.rg;
    pl.gs = c6.gs;
    pl.xcds = xcd_mask(d, c6, fwd);
    pl.xpd = pl.xcds ? 1 : 0;
    pl.scratch_free = rec6_scratch_free(rec6_kernel(fwd, d.mode, d.prec, d.H, c6));
  } else {
    pl.nth = NT;
    pl.lds = fwd ? fwd_lds_bytes(d, N, U) : bwd_lds_bytes(d, N, U);
    pl.xpd = gu.xpd;
  }
  pl.wgs = d.dirs * pl.nwg * pl.rg;
  // slot-mapped generic: eight XCD slots of nwg / xpd workgroups; pinned v6: eight of nwg
  pl.grid = !pl.xpd ? pl.wgs : c6 ? 8 * pl.nwg : 8 * ceil_div(pl.nwg, pl.xpd);
  return pl;
}

const void *rnn_rec6_select(const RnnDesc &d, int N, bool fwd, int cfg[5]) {
  const V6Cfg c = plan_rec(d, N, fwd).c6;
  cfg[0] = c.U, cfg[1] = c.nth, cfg[2] = c.rg, cfg[3] = c ? c.gs : 0, cfg[4] = c.variant;
  return c ? rec6_kernel(fwd, d.mode, d.prec, d.H, c) : nullptr;
}
void rnn_rec_plan(const RnnDesc &d, int N, bool fwd, long plan[8]) {
  const RecPlan p = plan_rec(d, N, fwd);
  plan[0] = p.ver, plan[1] = p.U, plan[2] = p.grid, plan[3] = p.nth, plan[4] = (long)p.lds, plan[5] = p.xcds,
  plan[6] = p.nwg, plan[7] = p.xpd;
}
size_t rnn_ws_colmax_offset(const RnnDesc &d, int T, int N) {
  const RnnWs ws(d, T, N, nullptr);
  return ws.pack_off + ws.lay.cme;
}

}  // namespace kctc
