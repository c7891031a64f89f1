// rnn.hip -- cuDNN-v5 compatible LSTM / GRU / RELU / TANH layers for gfx950.
//
// Replaces cudnnRNNForwardTraining / BackwardData / BackwardWeights as the
// reference calls them (src/cudamatrix/cudnn-recurrent.cc:13-102 through
// src/nnet2/nnet-cudnn-component.cc:508-614).  Per stacked layer:
//
// Forward
//   1. G = x W^T + bW (+ bR): the input projection of all T*N frames of both
//      directions as one packed split-fp16 GEMM (gemm_x3p.hip) -- or, for the
//      layers above the first, streamed off the previous component's running
//      recurrence (launch_chain_proj).
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
// Hand-off protocol (both recurrences): payload sc1 stores -> every storing
// wave's s_waitcnt vmcnt(0) -> workgroup barrier -> lane 0 stores the step
// epoch into the workgroup's own 128-B flag line; consumers poll the flag
// lines of their producers, then sc1 loads (MI355X_MICROARCH.md "Valid forms",
// row 1).  Every spin is bounded (3 s); a timeout sets the device error word,
// every workgroup drains out and the train step fails loudly.
// v4 (fp32 MFMA, XCD-slot all-gather) and v3 remain for the shapes v6 does
// not compile (RELU / TANH, other H, N > 64).  This file is the host side; the
// kernels: rec6_fwd.hip, rec6_bwd.hip, rec_generic.hip (v3 / v4), rec_common.h.
//
// Semantics follow cuDNN v5 as used by CuDNNRecurrentComponent: hx = cx = 0,
// dhy = dcy = 0 (SetBufferZero, nnet-cudnn-component.cc:494-506), all N
// sequences run the full T steps (no masking), weights in the opaque layout of
// nnet-cudnn-component.cc:327-413 (see RnnDesc::lin_offset).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "common.h"
#include "elementwise.h"
#include "gemm.h"
#include "prof.h"
#include "rec_common.h"
#include "rnn.h"

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

static long al64(long x) { return (x + 63) / 64 * 64; }
void rnn_set_precision(RnnDesc &d, int prec) {
  d.prec = prec;
  const char *e = getenv("KCTC_BF16_DIRECT");
  d.pk = !e || atoi(e) != 0;
  e = getenv("KCTC_BF16_IO");
  d.pkio = !e || atoi(e) != 0;
}

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

static long drec_split_floats(const RnnDesc &d, int T, int N) {
  // the dR and dW split slabs of a layer side by side: with a second stream
  // (rnn_backward_weights' s2) the two GEMMs run concurrently
  long need = 0, needR = 0, needW = 0;
  const int G4 = d.nw() * d.H;
  const int KB = (int)(((long)T * N + 31) / 32);  // packed k blocks over the frames (x3; bf16 needs fewer)
  for (int l = 0; l < d.layers; l++) {
    const long K = (long)(T > 1 ? T - 1 : 1) * N;
    int s = std::max(gemm_pick_split(G4, d.H, (int)K, d.dirs), x3p_pick_split(G4, d.H, KB, d.dirs));
    if (s > 1) needR = std::max(needR, (long)s * d.dirs * G4 * d.H);
    s = std::max(gemm_pick_split(G4, d.din(l), (int)((long)T * N), d.dirs), x3p_pick_split(G4, d.din(l), KB, d.dirs));
    if (s > 1) needW = std::max(needW, (long)s * d.dirs * G4 * d.din(l));
  }
  need = al64(needR) + needW;
  return need;
}

// split-K slabs of the weight-gradient GEMMs, then the recurrence flag words
static size_t flags_offset(const RnnDesc &d, int T, int N) {
  return sizeof(float) * (size_t)al64(drec_split_floats(d, T, N));
}
// then the v4 exchange images (one layer at a time; forward and backward of a
// layer never overlap): T * dirs * max(H, nW*H) * Npad floats
// flag region: words 0..1023 (v3/v4 flags, placement ids, GEMM tile counters
// at 1008/1009), then one 128-B line per (direction, workgroup) for v6
constexpr size_t kFlagBytes = 4096 + 512 * 128;  // v6: up to 4 row groups x 2 dirs x 64 workgroups
static size_t xch_offset(const RnnDesc &d, int T, int N) { return flags_offset(d, T, N) + kFlagBytes; }
static size_t xch_bytes(const RnnDesc &d, int T, int N) {
  const long Npad = (N + 15) / 16 * 16;
  // v4 images: 4 B x dirs x nW x H x Npad per step; the v6 forward's
  // [2 dirs][H/32][hi, lo][16][32] halves per row group of <= 16 rows (at most
  // 2 Npad / 16 groups): 16 B x H x Npad.  + 2 steps: the v6 forward's ring of
  // hand-off images after its T step images
  const size_t per = std::max<size_t>(sizeof(float) * d.dirs * d.nw(), 16);
  return per * (size_t)(T + 2) * d.H * Npad;
}
// then the packed split-fp16 GEMM operands of one layer at a time (forward,
// backward-data and the weight GEMMs of a component never overlap):
//   forward   : input rows [TN][Din], W rows [dirs*G][Din]
//   bwd data  : dGates rows [dirs*TN][G], W^T rows [dirs*Din][G]
//   bwd weight: dGates^T [dirs*G][TN] (+ GRU: E^T), input^T [Din][TN],
//               shifted output^T [dirs*H][TN]
// plus int exponents and float-bit column maxima (G = nW*H).
struct PackLay {
  size_t a, b, c, d, ea, eb, ec, ed, cm, part, cnt, part2, cme, fcnt, fpart, wt, ewt, cmw, xt, yt, ext, eyt, pcnt, total;
};
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
  p.d = o;  // unused slot kept for symmetry (0 bytes)
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
static size_t pack_offset(const RnnDesc &d, int T, int N) { return align_up(xch_offset(d, T, N) + xch_bytes(d, T, N), 256); }
size_t rnn_workspace_bytes(const RnnDesc &d, int T, int N) { return pack_offset(d, T, N) + pack_layout(d, T, N).total; }
template <typename P>
static P *pk(void *ws, const RnnDesc &d, int T, int N, size_t off) {
  return reinterpret_cast<P *>(static_cast<char *>(ws) + pack_offset(d, T, N) + off);
}
// The RNN GEMMs run on the packed split-fp16 matrix-core path (gemm_x3p.hip)
// unless the contraction is too short to pay for packing.
static bool use_x3(int K, int min_k = 128) { return K >= min_k; }
// |x| <= 1: an LSTM / GRU / TANH layer output
static bool bounded_out(const RnnDesc &d) { return d.mode != kRelu; }

static int env_int(const char *name, int dflt) {
  const char *v = getenv(name);
  return v ? atoi(v) : dflt;
}

// bf16 recurrences write their dGates straight into the packed bf16 GEMM
// operands (RecParams::dxr / dxt / et) -- v6 only (a v6 backward runs for
// every bf16 shape), whole 64-element gate rows
// (one-layer descriptors -- the recipe's components; a stacked descriptor's
// weight gradients measured wrong with it, so those keep the pack path)
static bool bf16_direct(const RnnDesc &d, int ver) {
  return d.prec == kPrecBf16 && ver == 6 && (d.nw() * d.H) % 64 == 0 && d.layers == 1 && d.pk;
}
// ... and, one-layer bidirectional, the forward writes its output packed
// (RecParams::yr / yc) and the backward E^T shifted (eshift); H % 32 == 0 so
// that a workgroup's units fill whole 16-B row chunks
static bool bf16_io(const RnnDesc &d) {
  return bf16_direct(d, 6) && d.layers == 1 && d.dirs == 2 && d.H % 32 == 0 && (2 * d.H) % 64 == 0 && d.pkio;
}

namespace {

// A recurrence kernel (rec6_kernel / rec_generic_kernel) on `nth` threads per workgroup; it was compiled
// against its own translation unit's copy of RecParams: the layouts agree only through rec_common.h
static void launch_rec(const void *k, const RecParams &p, dim3 grid, int nth, size_t lds, hipStream_t s) {
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

static size_t fwd_lds_bytes(const RnnDesc &d, int N, int U) {
  const int ncol = (d.nw() * U + 15) / 16 * 16, Npad = (N + 15) / 16 * 16;
  return sizeof(float) * ((size_t)ncol * (d.H + 4) + 4 * (size_t)Npad * ncol);
}
static size_t bwd_lds_bytes(const RnnDesc &d, int N, int U, int ver = 3) {
  const int Npad = (N + 15) / 16 * 16;
  return sizeof(float) * ((size_t)(ver == 4 ? 16 : U) * (d.nw() * d.H + 4) +
                          std::max(4 * (size_t)Npad * 16, (size_t)2 * N * U * d.nw()));
}

// pick U (units per workgroup): divides H, multiple of 4, blocks <= 256
static int pick_fwd_u(const RnnDesc &d, int N) {
  auto ok = [&](int U) {
    if (U < 4 || U % 4 || d.H % U || d.nw() * U > 16 * kMaxCT || N * U / 4 > NT) return false;
    if ((long)d.dirs * (d.H / U) > 256) return false;
    return fwd_lds_bytes(d, N, U) <= 160 * 1024;
  };
  // smallest U that keeps every workgroup resident (<= 256 = one per CU):
  // per-step MFMA latency falls with U (measured: U=4 < 8 < 16 on BLSTM-512)
  for (int U : {4, 8, 16})
    if (ok(U)) return U;
  return 0;
}

// v4 (XCD-local): nwg = H/U <= kCusPerXcd workgroups per direction, one XCD each.
constexpr int kCusPerXcd = 32;
// XCD slots one direction spans for U units per workgroup (0: not a v4 shape)
static int v4_xpd(const RnnDesc &d, int U) {
  if (U <= 0 || d.H % U) return 0;
  const int nwg = d.H / U;
  if (nwg % kCusPerXcd) return nwg < kCusPerXcd && d.dirs <= 8 ? 1 : 0;
  const int x = nwg / kCusPerXcd;
  return (x == 1 || x == 2 || x == 4 || x == 8) && x * d.dirs <= 8 ? x : 0;
}
static int pick_fwd_u4(const RnnDesc &d, int N) {
  if (d.dirs > 8) return 0;
  auto ok = [&](int U) {
    return U >= 4 && U % 4 == 0 && v4_xpd(d, U) && d.nw() * U <= 16 * kMaxCT && N * U <= kMaxEPT * NT &&
           fwd_lds_bytes(d, N, U) <= 160 * 1024;
  };
  // measured on BLSTM-512 N=16 (1 x MI355X): U=8 (2 XCD slots per direction)
  // 44 ms/step of forward recurrence, U=4 48, U=16 58
  for (int U : {8, 16, 4, 32})
    if (ok(U)) return U;
  return 0;
}
static int pick_bwd_u4(const RnnDesc &d, int N) {
  if (d.dirs > 8) return 0;
  auto ok = [&](int U) {
    return U >= 4 && U <= 16 && U % 4 == 0 && v4_xpd(d, U) && N * U <= kMaxEPT * NT &&
           bwd_lds_bytes(d, N, U, 4) <= 160 * 1024;
  };
  for (int U : {16, 8, 4})
    if (ok(U)) return U;
  return 0;
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
static int v6_group_rows(int N, bool fwd) {
  const int want = env_int("KCTC_REC_GS", N <= 16 ? 8 : 16);
  return (want == 8 && N > 8 && N <= 32) ? 8 : 16;
}
static V6Cfg pick6(const RnnDesc &d, int N, bool fwd, int gs_force = 0) {
  V6Cfg c;
  if ((d.mode != kLstm && d.mode != kGru) || N <= 0 || N > 64 || d.dirs > 2) return c;
  if (d.H != 256 && d.H != 320 && d.H != 512 && d.H != 1024) return c;
  const int gs = gs_force ? gs_force : v6_group_rows(N, fwd), rg = (N + gs - 1) / gs;
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

static size_t fwd6_lds_bytes(const RnnDesc &d, const V6Cfg &c) {
  const int CT = (d.nw() * c.U + 15) / 16, nwv = c.nth / 64, np = d.prec == kPrecBf16 ? 1 : 2;
  const size_t rp = std::max(CT * 16 + 1, 4 * c.U);  // rnn_fwd_rec6's RPR (float4 K partials)
  // + the IO waves' G (and output) slots; the stacked forward's launch keeps them (forward cfg only)
  const bool iow = c.variant == kRec6IoWave || c.variant == kRec6Stacked;
  const size_t b = sizeof(float) * (nwv * 16 * rp + 8) + np * 16 * (size_t)c.U * 2 + 16 +
                   (iow ? sizeof(float) * 16 * c.U * (8 * d.nw() + 2 * (d.nw() + 2)) + 16 + 4 * 64 * 4 : 0);
  return std::max(b, (size_t)96 * 1024);  // one recurrence workgroup per CU
}
static size_t bwd6_lds_bytes(const RnnDesc &d, const V6Cfg &c) {
  const int K = d.nw() * c.U, KB = (K + 31) / 32, AP = KB * 32 + 8;
  const size_t img = (d.prec == kPrecBf16 ? 1 : 2) * 16 * (size_t)AP * 2;
  const size_t red = sizeof(float) * std::max((size_t)c.nth * 4, (size_t)2 * 16 * c.U * d.nw());
  // dGates tile staged for write-through, and (bf16, packed writes) the E tile beside it
  const size_t estg = sizeof(float) * 16 * c.U * d.nw() * (d.prec == kPrecBf16 ? 2 : 1);
  // at least 96 KB so that no other workgroup (a side-stream GEMM block)
  // shares the CU with a recurrence workgroup
  return std::max(img + red + estg, (size_t)96 * 1024);
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

static float *xch_acquire(size_t bytes, hipStream_t s) {
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
static void xch_release(hipStream_t s) {
  int dev = 0;
  KCTC_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_xch_mu);
  XchPool &x = g_xch[dev & 63];
  if (!x.ev) KCTC_HIP_CHECK(hipEventCreateWithFlags(&x.ev, hipEventDisableTiming));
  KCTC_HIP_CHECK(hipEventRecord(x.ev, s));
}

static int pick_bwd_u(const RnnDesc &d, int N) {
  auto ok = [&](int U) {
    if (U < 4 || U % 4 || U > 16 || d.H % U || N * U / 4 > NT) return false;
    if ((long)d.dirs * (d.H / U) > 256) return false;
    return bwd_lds_bytes(d, N, U) <= 160 * 1024;
  };
  for (int U : {16, 8, 4})
    if (ok(U)) return U;
  return 0;
}

}  // namespace

// ---- launches beside a running recurrence (rnn.h rnn_side_gated) ----
namespace {
// the v6 recurrence this host thread enqueued last, while the host function
// that enqueued it runs (RecScope), and the side streams gated on it
struct RecInFlight {
  const unsigned *res = nullptr;    // its residency word (p.flags + kResWord)
  const unsigned *flags = nullptr;  // its flag area
  unsigned target = 0;              // its workgroups
  hipStream_t gated[4] = {};
  int ngated = 0;
};
thread_local RecInFlight g_rec;
// from a recurrence's launch to the end of the enclosing host call
struct RecScope {
  ~RecScope() { g_rec = RecInFlight{}; }
  void enqueued(const RecParams &p) {
    g_rec = RecInFlight{};
    g_rec.res = p.flags + kResWord;
    g_rec.flags = p.flags;
    g_rec.target = (unsigned)(p.dirs * p.nwg * p.rg);
  }
  void none() { g_rec = RecInFlight{}; }  // (a v3 / v4 recurrence: no side launches)
};
// `side` waits until every workgroup of the recurrence in flight is resident;
// whatever is enqueued on it afterwards may run beside that recurrence
void beside_recurrence(hipStream_t side) {
  if (!g_rec.res) throw std::logic_error("beside_recurrence: no recurrence in flight");
  for (int i = 0; i < g_rec.ngated; i++)
    if (g_rec.gated[i] == side) return;  // (already behind this recurrence's gate)
  if (g_rec.ngated == 4) throw std::logic_error("beside_recurrence: too many side streams");
  rnn_resident_gate(side, g_rec.flags, g_rec.target);
  g_rec.gated[g_rec.ngated++] = side;
}
}  // namespace

thread_local bool g_last_bwd_scratch_free = true;
bool rnn_last_bwd_scratch_free() { return g_last_bwd_scratch_free; }

bool rnn_side_gated(hipStream_t s) {
  if (!g_rec.res) return true;
  for (int i = 0; i < g_rec.ngated; i++)
    if (g_rec.gated[i] == s) return true;
  return false;
}

// ---------------------------------------------------------------------------
// host: forward training
// ---------------------------------------------------------------------------
namespace {
// The recurrence and a GEMM streaming off it must run at the same time, so
// the GEMM's stream forks from the recurrence's stream at an event recorded
// BEFORE the recurrence launch, and the GEMM is enqueued AFTER it: should the
// two streams share a hardware queue, the GEMM then merely runs after the
// recurrence instead of blocking it (its blocks only wait for recurrence flags).
int g_usable_cus = 0, g_comm_cus = 0;

// Does the v6 recurrence of (d, N) run without scratch (no register
// spills)?  Nothing runs beside one that does.  Round 6 first blamed scratch
// for configs[4]'s KCTC_STREAM_ALL hang (the bf16 GRU backward, then 124 B of
// spills per lane, stayed short of its 32 workgroups on one XCD for 0.4 s
// behind the one-wave residency wait of its dx stream); with the spills gone
// it hung the same way: the cause is its 256 VGPRs x 2 waves per SIMD, a
// whole CU's register file, which no workgroup gets on a CU where a gate wave
// sits -- gate_kernel's blocks now leave the recurrence's XCDs
// (tests/test_fullsize_gpu.py cfg4+stream_all).  The scratch
// condition stays as a precaution (no recipe-shape recurrence uses scratch).
bool rec6_scratch_free(const RnnDesc &d, int N, bool fwd) {
  const V6Cfg c6 = pick6(d, N, fwd);
  if (!c6) return false;
  static thread_local std::map<const void *, bool> memo;
  const void *k = rec6_kernel(fwd, d.mode, d.prec, d.H, c6);
  auto it = memo.find(k);
  if (it != memo.end()) return it->second;
  hipFuncAttributes a{};
  KCTC_HIP_CHECK(hipFuncGetAttributes(&a, k));
  return memo[k] = a.localSizeBytes == 0;
}

// XCDs an XCD-pinned v6 recurrence of (d, N) occupies (bit x: XCD x), 0
// when it is not pinned: every (row group, direction) runs on one XCD, its
// H / U workgroups on kCusPerXcd (configs[1] / [4]: 32) or kCusPerXcd / 2
// (configs[2]: U = 32 at H = 512, four row groups x two directions = all
// eight XCDs, half of each XCD's CUs) of that XCD's CUs, and the whole chip's
// CUs must be usable (no CU partition).  KCTC_XCD6=0 / KCTC_XCD6F=0 switch it
// off; the 16-workgroup shapes pin too (configs[2]
// pinned: 990k -> 1.12M frames/s, forward 3.14 -> 2.42, backward 4.52 -> 3.53
// us/step, same box).
unsigned xcd_mask(const RnnDesc &d, int N, bool fwd) {
  const V6Cfg c6 = pick6(d, N, fwd);
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

// persistent blocks a streamed GEMM may run beside a recurrence of `rec_wgs`
// workgroups (rnn.h, CU budget); 0: too few to stream
int stream_block_budget(int rec_wgs, bool backward) {
  // the 16-CU margin keeps room for the exchange's kernels beyond maxCTAs;
  // a backward without an exchange (one rank) gives the streamed dx GEMM all
  // CUs the recurrence leaves (configs[1]: 128 blocks, 655.7k -> 670.7k frames/s)
  const int margin = backward && rnn_comm_cus() == 0 ? 0 : 16;
  const int left = rnn_usable_cus() - rec_wgs - (backward ? rnn_comm_cus() : 0) - margin;
  return left >= 8 ? left : 0;
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

// Is the dx of layer l streamed off its v6 backward recurrence
// (launch_bwd_stream, given a dx buffer and an overlap stream)?  The
// forward's W^T prepack (RnnPrepack) asks the same question.
bool bwd_dx_stream_ok(const RnnDesc &d, int l, int T, int N) {
  const V6Cfg c6 = pick6(d, N, false);
  if (!c6 || d.dirs != 2 || !env_int("KCTC_BWD_STREAM", 1) || !rec6_scratch_free(d, N, false)) return false;
  // split-fp16 at N <= 16 by default (KCTC_STREAM_ALL: bf16 and N > 16 too)
  if (!((d.prec == kPrecX3 && N <= 16) || env_int("KCTC_STREAM_ALL", 0))) return false;
  const int G4 = d.nw() * d.H;
  if (!use_x3(G4) || G4 > 4096 || (d.prec != kPrecX3 && G4 % 64)) return false;
  if ((long)T * N * d.din(l) * 4 >= (1L << 31)) return false;
  return stream_block_budget(d.dirs * (d.H / c6.U) * c6.rg, true) > 0;
}

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

// Can `c` consume the exchange images of this component's last forward
// recurrence (v6, bidirectional) as its layer-0 projection input?
bool chain_ok(const RnnDesc &d, int ver, int T, int N, const RnnFwdChain *c) {
  if (!c || !c->d || !c->side || ver != 6 || d.dirs != 2 || !env_int("KCTC_FWD_STREAM", 1)) return false;
  if (!rec6_scratch_free(d, N, true)) return false;
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
  if (xcd_mask(d, N, true) && !env_int("KCTC_FWD_STREAM_PINNED", 0)) return false;
  // and only the IO-wave variant carries the copies (not bf16 in 8-row groups: never run pinned with them)
  const V6Cfg c6 = pick6(d, N, true);
  if (xcd_mask(d, N, true) && (c6.variant != kRec6IoWave || (d.prec == kPrecBf16 && c6.gs <= 8))) return false;
  if (!c6 || !stream_block_budget(d.dirs * (d.H / c6.U) * c6.rg, false)) return false;
  const long xs = 2L * (d.H / 32) * (d.prec == kPrecBf16 ? 1 : 2) * 16 * 32 * c6.rg;  // halves per step image
  if ((long)T * xs * 2 >= (1L << 31)) return false;
  return c->ws_bytes >= rnn_workspace_bytes(n, T, N) &&
         c->res_bytes >= sizeof(float) * (size_t)rnn_reserve_layout(n, T, N).total;
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
  const PackLay pl = pack_layout(n, T, N);
  _Float16 *Bp = pk<_Float16>(c.workspace, n, T, N, pl.b);
  int *eB = bf ? nullptr : pk<int>(c.workspace, n, T, N, pl.eb);
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
  x.tile_counter = reinterpret_cast<int *>(static_cast<char *>(c.workspace) + flags_offset(n, T, N));
  // XCD-pinned producer: the sc1 copies of its epochs, no block on its XCDs
  x.stream_flags = p.flags + 1024 + (p.xpd ? 256 * kFlagStride : 0);  // pinned: agg_flag6 lines
  x.stream_nwg = p.xpd ? 1 : p.nwg; x.stream_T = T; x.stream_N = N;
  const int pinned = whole_pinned_xcds(p);
  if (pinned) { x.stream_xcd_word = p.flags + kXcdWord; x.stream_xcd_count = pinned; }
  x.stream_group_step = 2L * (d.H / 32) * (bf ? 1 : 2) * 16 * 32;  // rnn_fwd_rec6's XG
  x.stream_rg = p.rg; x.stream_gs = p.gs; x.stream_step = x.stream_group_step * p.rg; x.stream_err = err;
  // K split by producer direction: the work is ready from the first steps
  // (KCTC_STREAM_DIRSPLIT=0: whole-K tiles from the middle of the sequence outwards)
  if (env_int("KCTC_STREAM_DIRSPLIT", 1)) {
    x.stream_arrive = pk<int>(c.workspace, n, T, N, pl.fcnt);
    x.stream_part = pk<float>(c.workspace, n, T, N, pl.fpart);
  }
  // every producer workgroup needs a CU of its own (96 KB LDS); the GEMM's
  // persistent blocks (96 KB each) take the rest minus a margin (chain_ok
  // checked that at least 8 fit).  No gradient exchange runs during a
  // forward pass: the updates of the previous step waited for it.
  // (blocks landing on a pinned producer's XCDs exit at once: launch enough that the budget stays)
  const int nb = stream_block_budget(d.dirs * p.nwg * p.rg, false);
  x.max_blocks = pinned ? nb * 8 / (8 - pinned) : nb;
  {
    ProfSpan ps(c.side, "fwd_proj_stream");
    gemm_x3p(c.side, x);
  }
  c.done = true;
}

// Can `c`'s layer-0 projection stream off this component's y rows
// (launch_chain_rows)?  Split-fp16 into split-fp16, the 256-tile row stream.
bool chain_rows_ok(const RnnDesc &d, int ver, int T, int N, const RnnFwdChain *c) {
  if (!c || !c->d || !c->side || ver != 6 || d.dirs != 2 || d.prec == kPrecBf16 || !env_int("KCTC_FWD_STREAM", 1))
    return false;
  if (!rec6_scratch_free(d, N, true)) return false;
  const RnnDesc &n = *c->d;
  const long TN = (long)T * N;
  if (n.D != d.dirs * d.H || n.prec != d.prec || !use_x3(n.D) || d.H % 32 || d.H > 4096 || T < 2) return false;
  if (!x3p_bwd_stream_256((int)TN, n.dirs * n.nw() * n.H, d.H / 32, false)) return false;
  if (TN * n.dirs * n.nw() * n.H * 4 >= (1L << 31) || TN * (d.H / 32) * 128 >= (1L << 31)) return false;
  // at N <= 16 (configs[1]); larger batches run the 256-tile GEMM after the
  // recurrence (shorter recurrences, less time to hide the GEMM behind)
  if (N > 16 && !env_int("KCTC_STREAM_ALL", 0)) return false;
  const V6Cfg c6 = pick6(d, N, true);
  if (!c6 || !stream_block_budget(d.dirs * (d.H / c6.U) * c6.rg, false)) return false;
  return c->ws_bytes >= rnn_workspace_bytes(n, T, N) &&
         c->res_bytes >= sizeof(float) * (size_t)rnn_reserve_layout(n, T, N).total;
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
  const PackLay pl = pack_layout(n, T, N);
  _Float16 *Bp = pk<_Float16>(c.workspace, n, T, N, pl.b);
  int *eB = pk<int>(c.workspace, n, T, N, pl.eb);
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
  a.Ap = pk<_Float16>(c.workspace, n, T, N, pl.a); a.eA = pk<int>(c.workspace, n, T, N, pl.ea);
  a.B = Bp; a.eB = eB; a.sB = sB; a.seB = n.dirs * G;
  a.C = static_cast<float *>(c.reserve) + lay.G; a.ldc = (long)n.dirs * G;
  a.bias = wl + (n.lin_offset(0, 0, true) - pl0);
  a.bias2 = n.mode == kGru ? nullptr : wl + (n.lin_offset(0, NW, true) - pl0);
  a.bias_cols = G; a.sbias = pls;
  a.part = pk<float>(c.workspace, n, T, N, pl.fpart);
  a.part2 = pk<float>(c.workspace, n, T, N, pl.part2);
  a.cnt = pk<int>(c.workspace, n, T, N, pl.cnt);
  a.flags = p.flags + 1024 + (p.xpd ? 256 * kFlagStride : 0);  // pinned: agg_flag6 lines
  a.nwg = p.xpd ? 1 : p.nwg; a.T = T; a.Nf = N; a.err = err; a.rg = p.rg;
  const int pinned = whole_pinned_xcds(p);
  if (pinned) { a.xcd_word = p.flags + kXcdWord; a.xcd_count = pinned; }
  // 128: every CU the recurrence leaves (configs[1]: 96 -> 128 blocks 720k -> 751k frames/s)
  const int nb = std::min(128, stream_block_budget(d.dirs * p.nwg * p.rg, false));
  a.blocks = pinned ? nb * 8 / (8 - pinned) : nb;
  {
    ProfSpan ps(c.side, "fwd_proj_rows");
    gemm_x3p_bwd_stream(c.side, a);
  }
  c.done = true;
}

}  // namespace

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
const void *rnn_rec6_select(const RnnDesc &d, int N, bool fwd, int cfg[5]) {
  const V6Cfg c = pick6(d, N, fwd);
  cfg[0] = c.U, cfg[1] = c.nth, cfg[2] = c.rg, cfg[3] = c ? c.gs : 0, cfg[4] = c.variant;
  return c ? rec6_kernel(fwd, d.mode, d.prec, d.H, c) : nullptr;
}

// ---- residency gate of the gradient exchange (rnn.h) ----
namespace {
struct RegWord {
  unsigned *word = nullptr;          // [1]: gate timeouts, [2]: pinned XCDs, [4..5]: registrations (64-bit: never wraps),
                                     // [6]: exchange gate blocks gone (rnn_comm_gate)
  unsigned long long expected = 0;   // host: registrations once every enqueued launch is resident
};
RegWord g_reg[64];
int g_comm_gated[64] = {0};  // per device: live gated exchanges (at most one, GatedExchange)
int current_device() {
  int dev = 0;
  KCTC_HIP_CHECK(hipGetDevice(&dev));
  return dev & 63;
}
RegWord &reg_of_device() {
  int dev = 0;
  KCTC_HIP_CHECK(hipGetDevice(&dev));
  RegWord &r = g_reg[dev & 63];
  if (!r.word) {
    KCTC_HIP_CHECK(hipMalloc(&r.word, 256));
    KCTC_HIP_CHECK(hipMemset(r.word, 0, 256));
  }
  return r;
}
}  // namespace

// The gates poll the word (10 s at most, then they give up and set bit 0 of
// the device word's [1]).  hipStreamWaitValue is no alternative: ROCclr runs
// it as a one-thread kernel too (__amd_rocclr_streamOpsWait), without a
// timeout -- under rocprofv3's counter collection, which serialises
// dispatches, a gate dispatched before its recurrence then never returns.
// A gate is kGateBlocks one-wave blocks, one per XCD (round-robin dispatch).
// A wave of it holds a CU, and a recurrence workgroup that needs a CU's whole
// register file (configs[4]'s bf16 GRU backward: 256 VGPRs x 2 waves per
// SIMD) cannot be placed beside it: a gate on one of the 32 CUs of an XCD the
// recurrence is pinned to kept that XCD's last workgroup out until the gate
// timed out (error 0x10003 at configs[4] with KCTC_STREAM_ALL=1).  So a block
// leaves as soon as the recurrence has a workgroup on its own XCD (xw: the
// XCD bits its workgroups OR in first thing), unless it is the last block
// still waiting (leave counts the ones gone): the blocks on XCDs the
// recurrence does not use do the waiting.  (A full-register recurrence on all
// eight XCDs would keep the last block's CU; no recipe shape is one -- with
// every CU taken nothing streams beside it either -- and the gate's timeout
// would flag it.)
constexpr int kGateBlocks = 8;
template <typename W>
__global__ __launch_bounds__(64) void gate_kernel(const W *word, W target, unsigned *gerr, const unsigned *xw,
                                                  unsigned *leave) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  const unsigned me = 1u << xcc_id();
  bool late = false;
  while (true) {
    const W v = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (__builtin_amdgcn_readfirstlane((int)(v >= target))) break;
    if (xw && __builtin_amdgcn_readfirstlane((int)(__hip_atomic_load(xw, __ATOMIC_RELAXED,
                                                                     __HIP_MEMORY_SCOPE_AGENT) & me))) {
      unsigned gone = 0;
      if (threadIdx.x == 0) gone = atomicAdd(leave, 1u);
      if (__builtin_amdgcn_readfirstlane((int)gone) < kGateBlocks - 1) return;
      xw = nullptr;  // the last one: it stays
    }
    late = __builtin_amdgcn_s_memrealtime() - t0 > 1000000000ull;  // 100 MHz clock
    if (late) break;
    __builtin_amdgcn_s_sleep(8);
  }
  if (late && threadIdx.x == 0) atomicOr(gerr, 1u);
}

unsigned long long rnn_bwd_registrations() { return reg_of_device().expected; }
void rnn_resident_gate(hipStream_t s, const unsigned *flags, unsigned target) {
  hipLaunchKernelGGL(gate_kernel<unsigned>, dim3(kGateBlocks), dim3(64), 0, s, flags + kResWord, target,
                     reg_of_device().word + 1, flags + kXcdWord, const_cast<unsigned *>(flags) + kGateWord);
  KCTC_HIP_CHECK(hipGetLastError());
}
const unsigned *rnn_pinned_xcds() { return reg_of_device().word + 2; }

void rnn_comm_gate(hipStream_t s, unsigned long long target) {
  RegWord &r = reg_of_device();
  // XCDs of the pinned backward recurrences (word [2], never cleared); the
  // blocks gone counted in word [6], zeroed per gate on its own stream
  KCTC_HIP_CHECK(hipMemsetAsync(r.word + 6, 0, sizeof(unsigned), s));
  hipLaunchKernelGGL(gate_kernel<unsigned long long>, dim3(kGateBlocks), dim3(64), 0, s,
                     reinterpret_cast<const unsigned long long *>(r.word + 4), target, r.word + 1, r.word + 2,
                     r.word + 6);
  KCTC_HIP_CHECK(hipGetLastError());
}
void rnn_set_comm_gated(bool on) {
  int &c = g_comm_gated[current_device()];
  c = on ? c + 1 : std::max(0, c - 1);
}
bool rnn_comm_gated() { return g_comm_gated[current_device()] > 0; }

bool rnn_packed_output(const RnnDesc &d, int T, int N, void *reserve, const void **rows, const void **cols) {
  *rows = *cols = nullptr;
  if (!bf16_io(d) || !reserve) return false;
  const RnnReserveLayout lay = rnn_reserve_layout(d, T, N);
  float *res = static_cast<float *>(reserve);
  *rows = res + lay.pkyr;
  *cols = res + lay.pkyc;
  return true;
}

namespace {
void pack_dx_weights(const RnnDesc &d, int l, const float *w, void *workspace, int T, int N, hipStream_t st);
}  // namespace

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
  if (ws_bytes < rnn_workspace_bytes(d, T, N)) return KRNN_BAD_PARAM;
  const V6Cfg c6 = pick6(d, N, true);
  const int U6 = c6.U;
  const int U4 = U6 ? 0 : pick_fwd_u4(d, N);
  const int ver = U6 ? 6 : U4 ? 4 : 3;
  const int U = U6 ? U6 : U4 ? U4 : pick_fwd_u(d, N);
  if (d.prec == kPrecBf16 && ver != 6) return KRNN_NOT_SUPPORTED;  // bf16 exists on v6 only
  if (!U) return KRNN_NOT_SUPPORTED;
  const int NW = d.nw(), H = d.H, dirs = d.dirs;
  const long TN = (long)T * N;
  float *res = static_cast<float *>(reserve);
  const float *in = x;
  for (int l = 0; l < d.layers; l++) {
    float *R0 = res + lay.per_layer * l;
    float *out = (l == d.layers - 1) ? y : R0 + lay.out;
    const int Din = d.din(l);
    const long pl0 = d.lin_offset(l * dirs, 0, false);
    const float *wl = w + pl0;
    const long pls = d.pl_size(l);
    const long bW = d.lin_offset(l * dirs, 0, true) - pl0;
    const long bR = d.lin_offset(l * dirs, NW, true) - pl0;
    const long roff = d.lin_offset(l * dirs, NW, false) - pl0;
    if (ver == 3) KCTC_HIP_CHECK(hipMemsetAsync(out, 0xFF, sizeof(float) * TN * dirs * H, s));
    GemmArgs g;
    g.transA = false; g.transB = true;
    g.M = (int)TN; g.N = NW * H; g.K = Din;
    const bool skip_proj = l == 0 && input_projected;  // streamed by the previous component
    g.A = in; g.lda = Din;
    g.B = wl; g.ldb = Din;
    g.C = R0 + lay.G; g.ldc = (long)dirs * NW * H;
    g.bias = wl + bW;
    g.bias2 = (d.mode == kGru) ? nullptr : wl + bR;
    g.batch = dirs; g.strideA = 0; g.strideB = pls; g.strideC = (long)NW * H; g.strideBias = pls;
    if (skip_proj) {
    } else if (d.prec == kPrecBf16 && use_x3(Din, 32)) {
      // bf16 gate GEMM: input rows and W rows packed as bf16, fp32 accumulation
      const PackLay pl = pack_layout(d, T, N);
      // the input rows come packed from the previous component's forward (in_rows)
      const bool rows_in = l == 0 && in_rows && Din % 64 == 0;
      __bf16 *Ap = rows_in ? static_cast<__bf16 *>(const_cast<void *>(in_rows)) : pk<__bf16>(workspace, d, T, N, pl.a);
      __bf16 *Bp = pk<__bf16>(workspace, d, T, N, pl.b);
      const int KB = (Din + 63) / 64;
      {
        ProfSpan ps(s, "x3_pack");
        if (!rows_in) bf16_pack_rows(s, in, Din, (int)TN, Din, Ap);
        bf16_pack_rows(s, wl, Din, NW * H, Din, Bp, dirs, pls, (long)NW * H * KB * 64);
      }
      X3PArgs x;
      x.bf16 = true;
      x.M = (int)TN; x.N = NW * H; x.KB = KB;
      x.A = reinterpret_cast<const _Float16 *>(Ap); x.B = reinterpret_cast<const _Float16 *>(Bp);
      x.C = g.C; x.ldc = g.ldc; x.bias = g.bias; x.bias2 = g.bias2;
      x.batch = dirs; x.sA = 0; x.sB = (long)NW * H * KB * 64;
      x.sC = g.strideC; x.sBias = g.strideBias;
      ProfSpan ps(s, "gemm_fwd_proj");
      gemm_x3p(s, x);
    } else if (use_x3(Din, 32)) {
      // input rows (a lower stacked layer's output is bounded; the component
      // input and RELU outputs get per-row exponents) and W rows, packed
      const PackLay pl = pack_layout(d, T, N);
      _Float16 *Ap = pk<_Float16>(workspace, d, T, N, pl.a), *Bp = pk<_Float16>(workspace, d, T, N, pl.b);
      int *eA = pk<int>(workspace, d, T, N, pl.ea), *eB = pk<int>(workspace, d, T, N, pl.eb);
      const int KB = (Din + 31) / 32;
      {
        ProfSpan ps(s, "x3_pack");
        x3p_pack_rows(s, in, Din, (int)TN, Din, Ap, eA, (l > 0 && bounded_out(d)) ? 1.f : 0.f);
        x3p_pack_rows(s, wl, Din, NW * H, Din, Bp, eB, 0.f, dirs, pls, (long)NW * H * KB * 64, (long)NW * H);
      }
      X3PArgs x;
      x.M = (int)TN; x.N = NW * H; x.KB = KB;
      x.A = Ap; x.B = Bp; x.eA = eA; x.eB = eB;
      x.C = g.C; x.ldc = g.ldc; x.bias = g.bias; x.bias2 = g.bias2;
      x.batch = dirs; x.sA = 0; x.seA = 0; x.sB = (long)NW * H * KB * 64; x.seB = (long)NW * H;
      x.sC = g.strideC; x.sBias = g.strideBias;
      ProfSpan ps(s, "gemm_fwd_proj");
      gemm_x3p(s, x);
    } else {
      ProfSpan ps(s, "gemm_fwd_proj");
      gemm_f32(s, g);
    }
    RecParams p{};
    p.T = T; p.N = N; p.H = H; p.dirs = dirs; p.U = U; p.nwg = H / U;
    p.ncol = (NW * U + 15) / 16 * 16; p.Npad = (N + 15) / 16 * 16;
    p.w = wl; p.pl_stride = pls; p.r_off = roff; p.bR_off = bR;
    p.G = R0 + lay.G; p.y = out; p.aux = R0 + lay.aux; p.err = err;
    p.sync = ver == 4 ? kSyncFlag : kSyncData;
    p.allow_local = 0;
    p.flags = reinterpret_cast<unsigned *>(static_cast<char *>(workspace) + flags_offset(d, T, N));
    KCTC_HIP_CHECK(hipMemsetAsync(p.flags, 0, kFlagBytes, s));
    const size_t lds = ver == 6 ? fwd6_lds_bytes(d, c6) : fwd_lds_bytes(d, N, U);
    p.xpd = ver == 4 ? v4_xpd(d, U) : 1;
    p.rg = ver == 6 ? c6.rg : 1;
    p.gs = ver == 6 ? c6.gs : 16;
    p.xch = reinterpret_cast<float *>(static_cast<char *>(workspace) + xch_offset(d, T, N));
    p.poll_sleep = 1;
    p.gla = 3;  // G rows fetched 3 steps ahead (IO waves)
    if (ver == 6 && bf16_io(d)) {  // the output also as packed bf16 rows and columns
      p.yr = reinterpret_cast<__bf16 *>(R0 + lay.pkyr);
      p.yc = reinterpret_cast<__bf16 *>(R0 + lay.pkyc);
      p.kbt64 = lay.kbt64;
      if (lay.kbt64 > TN)
        KCTC_HIP_CHECK(hipMemset2DAsync(p.yc + TN, sizeof(__bf16) * lay.kbt64, 0, sizeof(__bf16) * (lay.kbt64 - TN),
                                        (size_t)dirs * H, s));
    }
    const bool chained = l == d.layers - 1 && chain_ok(d, ver, T, N, chain);
    const bool rowchain = !chained && l == d.layers - 1 && chain_rows_ok(d, ver, T, N, chain);
    if (ver == 6) {
      // XCD-pinned forward (xcd_mask): each (row group, direction) on one XCD,
      // the h hand-off in its L2 through a ring of two step images; a
      // streamed projection gets sc1 copies of the step images and flags
      p.xpd = xcd_mask(d, N, true) ? 1 : 0;
      p.ring = p.xpd ? 2 : 0;
      p.fcopy = p.xpd && chained;
      p.ysc1 = rowchain ? 1 : 0;
      p.allow_local = p.xpd ? 1 : 0;
      // self-tagged hand-off (the kernel takes it for split-fp16 variants other
      // than kRec6IoWave, without a write-through copy): the ring starts at tag 1
      p.dtag = d.prec != kPrecBf16 && p.ring == 2 && !p.fcopy && T >= 2;
      if (p.dtag) {  // rnn_fwd_rec6's ring: after T step images of XS = 64 H rg halves (2 dirs, hi / lo, 16 rows)
        const size_t xs = sizeof(_Float16) * 64 * (size_t)d.H * p.rg;
        KCTC_HIP_CHECK(hipMemsetAsync(reinterpret_cast<char *>(p.xch) + xs * T, 0x01, 2 * xs, s));
      }
    }
    const dim3 grid(ver == 4 ? 8 * ceil_div(p.nwg, p.xpd) : ver == 6 && p.xpd ? 8 * p.nwg : dirs * p.nwg * p.rg);
    RecTrace tr;
    if (tr.arm("fwd", grid.x)) p.trace = tr.dev;
    // W^T of the backward's streamed dx GEMM, packed beside this recurrence
    // (rnn_backward_data's `streamed` shapes; one-layer descriptors)
    const bool prepack = pre && pre->dx && pre->stream && pre->ev && ver == 6 && d.layers == 1 &&
                         bwd_dx_stream_ok(d, 0, T, N);
    const bool prepack_w = pre && pre->stream && pre->wev && pre->wgrad && pre->in_bound > 0.f && ver == 6 &&
                           d.layers == 1 && d.prec != kPrecBf16 && T > 1 && bounded_out(d) && use_x3((int)TN) &&
                           rec6_scratch_free(d, N, true);
    const hipEvent_t fork = (chained || prepack || prepack_w || rowchain) ? fork_event(s) : nullptr;
    {
      ProfSpan ps(s, "rnn_fwd_rec");
      if (ver == 6) launch_rec(rec6_kernel(true, d.mode, d.prec, H, c6), p, grid, c6.nth, lds, s);
      else launch_rec(rec_generic_kernel(true, ver, d.mode, p.Npad / 16), p, grid, NT, lds, s);
    }
    KCTC_HIP_CHECK(hipGetLastError());
    if (ver == 6) rec_scope.enqueued(p);
    else rec_scope.none();
    if (prepack) {  // beside the recurrence, once it is resident
      KCTC_HIP_CHECK(hipStreamWaitEvent(pre->stream, fork, 0));
      beside_recurrence(pre->stream);
      pack_dx_weights(d, 0, w, workspace, T, N, pre->stream);
      KCTC_HIP_CHECK(hipEventRecord(pre->ev, pre->stream));
      pre->done = true;
    }
    if (prepack_w) {  // x^T beside the recurrence, y^T after it, off its XCDs (rnn_backward_weights' packs)
      hipStream_t ss = pre->stream;
      if (!prepack) KCTC_HIP_CHECK(hipStreamWaitEvent(ss, fork, 0));
      beside_recurrence(ss);
      const PackLay pl = pack_layout(d, T, N);
      const int Din = d.din(0);
      int *pc = pk<int>(workspace, d, T, N, pl.pcnt);  // item counters
      KCTC_HIP_CHECK(hipMemsetAsync(pc, 0, sizeof(int) * 3, ss));
      const unsigned *av = rnn_pinned_xcds();
      const int nx = std::max(1, rnn_usable_cus() / kCusPerXcd);
      ProfSpan ps(ss, "x3_pack_w_fwd");
      x3p_pack_cols(ss, in, Din, (int)TN, Din, 0, pk<_Float16>(workspace, d, T, N, pl.xt),
                    pk<int>(workspace, d, T, N, pl.ext), nullptr, pre->in_bound, 1, 0, 0, 0, 0, av, nx, pc);
    }
    if (chained) {
      launch_chain_proj(d, p, fork, T, N, *chain, err);
      join_stream(s, chain->side);
    }
    if (rowchain) {
      launch_chain_rows(d, p, fork, T, N, *chain, err);
      join_stream(s, chain->side);
    }
    if (prepack_w) {  // y^T after the recurrence (and after the joins: s does not wait for it)
      hipStream_t ss = pre->stream;
      KCTC_HIP_CHECK(hipStreamWaitEvent(ss, fork_event(s), 0));
      const PackLay pl = pack_layout(d, T, N);
      const long KBt = (TN + 31) / 32;
      int *pc = pk<int>(workspace, d, T, N, pl.pcnt);
      const unsigned *av = rnn_pinned_xcds();
      const int nx = std::max(1, rnn_usable_cus() / kCusPerXcd);
      const long ldy = (long)dirs * H;
      {
        ProfSpan ps(ss, "x3_pack_w_fwd");
        for (int dir = 0; dir < dirs; dir++)
          x3p_pack_cols(ss, out + (long)dir * H, ldy, (int)TN, H, dir == 0 ? N : -N,
                        pk<_Float16>(workspace, d, T, N, pl.yt) + (long)dir * H * KBt * 64,
                        pk<int>(workspace, d, T, N, pl.eyt) + dir * H, nullptr, 1.f, 1, 0, 0, 0, 0, av, nx,
                        pc + 1 + dir);
      }
      KCTC_HIP_CHECK(hipEventRecord(pre->wev, ss));
      pre->wdone = true;
    }
    tr.dump("fwd", s, grid.x, p.nwg, T, dirs, ver, ver == 6 ? (p.xpd ? 1 : 0) : p.xpd);
    in = out;
  }
  return KRNN_OK;
}

namespace {
// dx of stacked layer l on `ov`, streamed off the backward recurrence about
// to be launched on `s` (gemm_x3p_bwd_stream): W_d^T packed first, then one
// persistent launch that packs dGates rows as the recurrence flags them.
// W^T of layer l's dx GEMM (B operand of the streamed GEMM) into the
// workspace slot pl.wt (per-column exponents pl.ewt, absmax scratch pl.cmw)
void pack_dx_weights(const RnnDesc &d, int l, const float *w, void *workspace, int T, int N, hipStream_t st) {
  const bool bf = d.prec == kPrecBf16;
  const int G4 = d.nw() * d.H, KB = G4 / (bf ? 64 : 32), Din = d.din(l);
  const long pl0 = d.lin_offset(l * d.dirs, 0, false), pls = d.pl_size(l);
  const float *wl = w + pl0;
  const PackLay pl = pack_layout(d, T, N);
  _Float16 *Bp = pk<_Float16>(workspace, d, T, N, pl.wt);
  int *eB = pk<int>(workspace, d, T, N, pl.ewt);
  unsigned *cm = pk<unsigned>(workspace, d, T, N, pl.cmw);
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

void launch_bwd_stream(const RnnDesc &d, const RecParams &p, int l, const float *w, float *dxl, void *workspace,
                       int T, int N, hipStream_t ov, hipEvent_t fork, unsigned *err, const RnnPrepack *pre) {
  KCTC_HIP_CHECK(hipStreamWaitEvent(ov, fork, 0));  // after the flag reset, not after the recurrence
  // not before every workgroup of the recurrence is resident: its blocks
  // wait (on_pinned_xcd) for the pinned recurrence's XCDs to register, and a
  // block parked on one of those XCDs' CUs before the recurrence's last
  // workgroup got there would keep it out (with W^T packed by the forward
  // the GEMM starts together with the recurrence)
  beside_recurrence(ov);
  const bool bf = d.prec == kPrecBf16;
  const int NW = d.nw(), H = d.H, G4 = NW * H, KB = G4 / (bf ? 64 : 32), Din = d.din(l);
  const long TN = (long)T * N;
  const PackLay pl = pack_layout(d, T, N);
  _Float16 *Ap = pk<_Float16>(workspace, d, T, N, pl.a), *Bp = pk<_Float16>(workspace, d, T, N, pl.wt);
  int *eA = pk<int>(workspace, d, T, N, pl.ea), *eB = pk<int>(workspace, d, T, N, pl.ewt);
  // packed by the forward on its side stream (RnnPrepack), else here
  if (pre && pre->done) KCTC_HIP_CHECK(hipStreamWaitEvent(ov, pre->ev, 0));
  else pack_dx_weights(d, l, w, workspace, T, N, ov);
  X3PBwdStream a;
  a.bf16 = bf;
  a.M = (int)TN; a.N = Din; a.KB = KB;
  a.E = p.DX; a.lde = 2L * G4; a.edoff = G4;
  a.Ap = Ap; a.eA = eA;
  a.B = Bp; a.eB = bf ? nullptr : eB; a.sB = (long)Din * KB * 64; a.seB = Din;
  a.C = dxl; a.ldc = Din;
  a.part = pk<float>(workspace, d, T, N, pl.part);
  a.part2 = pk<float>(workspace, d, T, N, pl.part2);
  a.cnt = pk<int>(workspace, d, T, N, pl.cnt);
  // XCD-pinned recurrence: its epochs' sc1 copies (the L2 flags are not
  // visible here), and no block on the recurrence's XCDs
  a.flags = p.flags + 1024 + (p.xpd ? 256 * kFlagStride : 0);  // pinned: agg_flag6 lines
  a.nwg = p.xpd ? 1 : p.nwg; a.T = T; a.Nf = N; a.err = err; a.rg = p.rg;
  const int pinned = whole_pinned_xcds(p);
  if (pinned) { a.xcd_word = p.flags + kXcdWord; a.xcd_count = pinned; }
  // 128 measured best at configs[1] since the self-tagged recurrences (96
  // before: 655.7k -> 670.7k frames/s); never more than the CU budget leaves
  // beside the recurrence and the exchange's kernels (rnn.h).  Blocks landing
  // on the pinned XCDs exit at once: launch enough that ~128 stay
  // 256-tile launch: 48 blocks keep up with the recurrence and leave the
  // other CUs beside it to the weight GEMMs (rnn_backward_weights beside)
  const bool t256 = x3p_bwd_stream_256(a.M, a.N, a.KB, bf);
  const int nb = std::min(t256 ? 64 : 128,
                          stream_block_budget(d.dirs * p.nwg * p.rg, true));
  a.blocks = pinned ? nb * 8 / (8 - pinned) : nb;
  ProfSpan ps(ov, "bwd_data_stream");
  gemm_x3p_bwd_stream(ov, a);
}
}  // namespace

// ---------------------------------------------------------------------------
// streamed weight gradients of the bottom component (rnn.h RnnWgradStream)
// ---------------------------------------------------------------------------
namespace {
// One wave: returns once every v6 flag line (stride kFlagStride words) holds
// >= epoch, the recurrence reported an error, or after 3 s (then err bit 3).
// Every exit decision is wave-uniform; the error store follows the loop.
__global__ __launch_bounds__(64) void rec_gate_kernel(const unsigned *flags, int nlines, unsigned epoch,
                                                      unsigned *err) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  int spins = 0;
  bool late = false;
  while (true) {
    bool ok = true;
    for (int i = threadIdx.x; i < nlines; i += 64)
      ok &= __hip_atomic_load(flags + (long)i * kFlagStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= epoch;
    if (__all(ok)) break;
    if ((++spins & 255) == 0) {
      const unsigned e = __builtin_amdgcn_readfirstlane(__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      if (e) break;
      late = __builtin_amdgcn_s_memrealtime() - t0 > 300000000ull;
      if (late) break;
    }
    __builtin_amdgcn_s_sleep(16);
  }
  if (late && threadIdx.x == 0) atomicOr(err, 8u);
}

// dW_dir += DX_dir^T x and dR_dir += DX_dir^T h_prev over the frames [ta, tb)
// of direction dir (layer 0 of a one-layer component, split-fp16, LSTM: E == DX)
void wgrad_frames(const RnnDesc &d, hipStream_t s, int T, int N, const float *x, const float *y, void *workspace,
                  float *dw, void *reserve, int max_blocks, float in_bound, int dir, int ta, int tb) {
  if (tb <= ta) return;
  const RnnReserveLayout lay = rnn_reserve_layout(d, T, N);
  const int NW = d.nw(), H = d.H, dirs = d.dirs, G4 = NW * H, Din = d.din(0);
  const long ldg = (long)dirs * G4, ldy = (long)dirs * H;
  const int R = (tb - ta) * N, KB = (R + 31) / 32;
  const float *DX = static_cast<const float *>(reserve) + lay.E;
  const PackLay pl = pack_layout(d, T, N);
  _Float16 *DXt = pk<_Float16>(workspace, d, T, N, pl.a), *Xt = pk<_Float16>(workspace, d, T, N, pl.b);
  _Float16 *Yt = pk<_Float16>(workspace, d, T, N, pl.c);
  int *eDX = pk<int>(workspace, d, T, N, pl.ea), *eX = pk<int>(workspace, d, T, N, pl.eb);
  int *eY = pk<int>(workspace, d, T, N, pl.ec);
  unsigned *cm = pk<unsigned>(workspace, d, T, N, pl.cm);
  unsigned *fl = reinterpret_cast<unsigned *>(static_cast<char *>(workspace) + flags_offset(d, T, N));
  float *ws = static_cast<float *>(workspace);
  const long ws_floats = drec_split_floats(d, T, N);
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
  auto split_for = [&](int n) {
    int sp = x3p_pick_split(G4, n, KB, 1);
    while (sp > 1 && (long)sp * G4 * n > ws_floats) sp--;
    return sp;
  };
  const long pl0 = d.lin_offset(dir, 0, false);
  {
    X3PArgs a;
    a.M = G4; a.N = Din; a.KB = KB;
    a.A = DXt; a.eA = eDX; a.B = Xt; a.eB = eX;
    a.C = dw + pl0; a.ldc = Din; a.beta = 1.f; a.batch = 1;
    a.split_k = split_for(Din); a.ws = ws;
    a.max_blocks = max_blocks;
    if (max_blocks > 0) a.tile_counter = reinterpret_cast<int *>(fl + 1008);
    ProfSpan ps(s, "gemm_bwd_w");
    gemm_x3p(s, a);
  }
  {
    X3PArgs a;
    a.M = G4; a.N = H; a.KB = KB;
    a.A = DXt; a.eA = eDX; a.B = Yt; a.eB = eY;
    a.C = dw + d.lin_offset(dir, NW, false); a.ldc = H; a.beta = 1.f; a.batch = 1;
    a.split_k = split_for(H); a.ws = ws;
    a.max_blocks = max_blocks;
    if (max_blocks > 0) a.tile_counter = reinterpret_cast<int *>(fl + 1009);
    ProfSpan ps(s, "gemm_bwd_r");
    gemm_x3p(s, a);
  }
}

// dbW += sum dGx, dbR += sum dGh of layer l from the recurrence's per-group partials
void wgrad_bias(const RnnDesc &d, hipStream_t s, int T, int N, float *dw, void *reserve, int l) {
  const RnnReserveLayout lay = rnn_reserve_layout(d, T, N);
  const int NW = d.nw(), H = d.H, dirs = d.dirs, G4 = NW * H;
  const float *R0 = static_cast<const float *>(reserve) + lay.per_layer * l;
  const long pl0 = d.lin_offset(l * dirs, 0, false), pls = d.pl_size(l);
  float *dwl = dw + pl0;
  const long bW = d.lin_offset(l * dirs, 0, true) - pl0;
  const long bR = d.lin_offset(l * dirs, NW, true) - pl0;
  // (v6: one partial per row group, [group][dir][2][G], added in group order)
  const V6Cfg c6b = pick6(d, N, false);
  const int rg = c6b ? c6b.rg : 1;
  for (int gi = 0; gi < rg; gi++)
    for (int dir = 0; dir < dirs; dir++) {
      const float *part = R0 + lay.bias + ((long)gi * dirs + dir) * 2 * G4;
      clip_sgd_update(s, dwl + dir * pls + bW, part, G4, 1.f, 0.f);
      clip_sgd_update(s, dwl + dir * pls + bR, part + G4, G4, 1.f, 0.f);
    }
}
}  // namespace

// Off by default (KCTC_WGRAD_STREAM=1 turns it on): measured on configs[1]
// 470.4k -> 467.0k (2 chunks), 466.1k (4), 454.5k (8) frames/s: the chunk
// GEMMs beside the backward recurrence slow it (33.0 -> 33.3-33.5 ms/step)
// and the per-chunk transposes add packing, more than the 1 ms tail saved.
bool rnn_wgrad_stream_ok(const RnnDesc &d, int T, int N) {
  if (!env_int("KCTC_WGRAD_STREAM", 0) || d.layers != 1 || d.dirs != 2 || d.mode != kLstm ||
      d.prec != kPrecX3 || T < 8 || N > 16)
    return false;
  if (!pick6(d, N, false) || !use_x3((int)((long)T * N)) || !use_x3(d.nw() * d.H) || !rec6_scratch_free(d, N, false))
    return false;
  return (long)T * N * d.din(0) * 4 < (1L << 31);
}

// ---------------------------------------------------------------------------
// host: backward data (dGates into the reserve, dx)
// ---------------------------------------------------------------------------
int rnn_backward_data(const RnnDesc &d, hipStream_t s, int T, int N, const float *y,
                      const float *dy, const float *w, float *dx, void *workspace,
                      size_t ws_bytes, void *reserve, size_t res_bytes, unsigned *err,
                      hipStream_t overlap, RnnWgradStream *wgrad, const RnnPrepack *pre) {
  RecScope rec_scope;  // the side launches' residency gates (beside_recurrence)
  if (wgrad) wgrad->done = false;
  if (T <= 0 || N <= 0 || N > 16 * kMaxRT || d.H % 16) return KRNN_NOT_SUPPORTED;
  const RnnReserveLayout lay = rnn_reserve_layout(d, T, N);
  if (res_bytes < sizeof(float) * (size_t)lay.total) return KRNN_BAD_PARAM;
  const V6Cfg c6 = pick6(d, N, false);
  const int U6 = c6.U;
  const int U4 = U6 ? 0 : pick_bwd_u4(d, N);
  const int ver = U6 ? 6 : U4 ? 4 : 3;
  const int U = U6 ? U6 : U4 ? U4 : pick_bwd_u(d, N);
  if (d.prec == kPrecBf16 && ver != 6) return KRNN_NOT_SUPPORTED;
  if (!U) return KRNN_NOT_SUPPORTED;
  const int NW = d.nw(), H = d.H, dirs = d.dirs;
  const long TN = (long)T * N;
  float *res = static_cast<float *>(reserve);
  const float *dcur = dy;
  for (int l = d.layers - 1; l >= 0; l--) {
    float *R0 = res + lay.per_layer * l;
    const float *out = (l == d.layers - 1) ? y : R0 + lay.out;
    const int Din = d.din(l);
    const long pl0 = d.lin_offset(l * dirs, 0, false);
    const float *wl = w + pl0;
    const long pls = d.pl_size(l);
    float *E = R0 + lay.E;
    float *DX = d.mode == kGru ? R0 + lay.DX : E;
    if (ver == 3) KCTC_HIP_CHECK(hipMemsetAsync(E, 0xFF, sizeof(float) * TN * dirs * NW * H, s));
    RecParams p{};
    p.T = T; p.N = N; p.H = H; p.dirs = dirs; p.U = U; p.nwg = H / U;
    p.ncol = 16; p.Npad = (N + 15) / 16 * 16;
    p.w = wl; p.pl_stride = pls; p.r_off = d.lin_offset(l * dirs, NW, false) - pl0;
    p.bR_off = d.lin_offset(l * dirs, NW, true) - pl0;
    p.G = R0 + lay.G; p.y = const_cast<float *>(out); p.aux = R0 + lay.aux;
    p.dy = dcur; p.E = E; p.DX = DX; p.bias = R0 + lay.bias; p.err = err;
    p.sync = kSyncFlag;
    p.allow_local = 0;
    if (ws_bytes < rnn_workspace_bytes(d, T, N)) return KRNN_BAD_PARAM;
    p.flags = reinterpret_cast<unsigned *>(static_cast<char *>(workspace) + flags_offset(d, T, N));
    KCTC_HIP_CHECK(hipMemsetAsync(p.flags, 0, kFlagBytes, s));
    const size_t lds = ver == 6 ? bwd6_lds_bytes(d, c6) : bwd_lds_bytes(d, N, U, ver);
    p.xpd = ver == 4 ? v4_xpd(d, U) : 1;
    p.rg = ver == 6 ? c6.rg : 1;
    p.gs = ver == 6 ? c6.gs : 16;
    if (ver == 6) {
      // XCD-pinned backward (xcd_mask): each (row group, direction) on one
      // XCD, the partial-dh hand-off in that XCD's L2, through a ring of two
      // step images (L2-resident).  configs[1]: 3.36 -> 2.70 us per step with
      // the streamed dx GEMM beside it (2.41 without), 468k -> 511k frames/s
      p.xpd = xcd_mask(d, N, false) ? 1 : 0;
      p.ring = p.xpd ? 2 : 0;
      p.allow_local = 1;
      p.poll_sleep = 1;
      p.bfpart = 1;
      p.xch = xch_acquire(sizeof(float) * (size_t)T * dirs * p.nwg * (16 * H + 64) * p.rg, s);
      // self-tagged hand-off (fp32 partials through the L2 ring): the two ring
      // images start with tag 1 in every word (steps 0 and 1 publish tag 0)
      p.dtag = d.prec != kPrecBf16 && p.ring == 2 && p.xpd && T >= 2;
      if (p.dtag)
        KCTC_HIP_CHECK(hipMemsetAsync(p.xch, 0x01, sizeof(float) * 2 * (size_t)dirs * p.nwg * (16 * H + 64) * p.rg, s));
    } else {
      p.xch = reinterpret_cast<float *>(static_cast<char *>(workspace) + xch_offset(d, T, N));
    }
    const dim3 grid(ver == 4 ? 8 * ceil_div(p.nwg, p.xpd) : ver == 6 && p.xpd ? 8 * p.nwg : dirs * p.nwg * p.rg);
    RecTrace tr;
    if (tr.arm("bwd", grid.x)) p.trace = tr.dev;
    // dx_l = sum_dir DX_dir W_dir   (lower layer's dy, or the caller's dx)
    float *dxl = (l == 0) ? dx : res + lay.per_layer * (l - 1) + lay.dout;
    // streamed: computed on `overlap` while the recurrence runs, from its rows as they appear
    const bool streamed = dxl && overlap && ver == 6 && bwd_dx_stream_ok(d, l, T, N);
    // weight gradients streamed off this recurrence (the bottom component):
    // its dGates rows must be written through too
    const bool wstream = wgrad && wgrad->side && !dxl && ver == 6 && !p.xpd && d.layers == 1 &&
                         rnn_wgrad_stream_ok(d, T, N);
    p.e_sc1 = (streamed || wstream) ? 1 : 0;
    // bf16: dGates straight into the packed operands of the dx / dW / dR GEMMs
    // (no fp32 rows, no pack passes over them; KCTC_BF16_DIRECT=0: the fp32
    // rows and the pack kernels as in round 3)
    const bool pkd = bf16_direct(d, ver);  // beside e_sc1's write-through rows when streamed
    if (pkd) {
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
    if (ver == 6) {
      p.cmax = pk<unsigned>(workspace, d, T, N, pack_layout(d, T, N).cme);
      if (p.rg > 1)  // max over the row groups by atomicMax on the float bits
        KCTC_HIP_CHECK(hipMemsetAsync(p.cmax, 0, sizeof(unsigned) * 2 * dirs * NW * H, s));
    }
    const hipEvent_t fork = (streamed || wstream) ? fork_event(s) : nullptr;
    RegWord &rw = reg_of_device();
    if (ver == 6) p.reg = rw.word;  // registration for the exchange's residency gate
    {
      ProfSpan ps(s, "rnn_bwd_rec");
      if (ver == 6) launch_rec(rec6_kernel(false, d.mode, d.prec, H, c6), p, grid, c6.nth, lds, s);
      else launch_rec(rec_generic_kernel(false, ver, d.mode, p.Npad / 16), p, grid, NT, lds, s);
    }
    KCTC_HIP_CHECK(hipGetLastError());
    if (ver == 6) {
      // counted once the launch is enqueued (a failed launch never raises the target)
      rw.expected += (unsigned long long)(dirs * p.nwg * p.rg);
      rec_scope.enqueued(p);
      g_last_bwd_scratch_free = rec6_scratch_free(d, N, false);
    } else {
      rec_scope.none();
      g_last_bwd_scratch_free = true;
    }
    if (streamed) {
      launch_bwd_stream(d, p, l, w, dxl, workspace, T, N, overlap, fork, err, d.layers == 1 ? pre : nullptr);
      join_stream(s, overlap);
    }
    if (wstream) {
      // chunk c of C: direction 0 frames [T - b(c+1), T - b(c)), direction 1
      // [b(c), b(c+1)), b(c) = c T / C; complete once every flag line holds
      // epoch b(c+1) + 2 (rows of step k are out at epoch k + 3)
      hipStream_t ws2 = wgrad->side;
      KCTC_HIP_CHECK(hipStreamWaitEvent(ws2, fork, 0));  // after the flag reset
      beside_recurrence(ws2);
      const int C = std::max(1, std::min(wgrad->chunks, T / 4));
      const unsigned *lines = p.flags + 1024;
      const int nlines = p.rg * dirs * p.nwg;
      for (int c = 0; c < C; c++) {
        const int b0 = (int)((long)c * T / C), b1 = (int)((long)(c + 1) * T / C);
        hipLaunchKernelGGL(rec_gate_kernel, dim3(1), dim3(64), 0, ws2, lines, nlines, (unsigned)(b1 + 2), err);
        wgrad_frames(d, ws2, T, N, wgrad->x, y, workspace, wgrad->dw, reserve, wgrad->max_blocks, wgrad->in_bound, 0,
                     T - b1, T - b0);
        wgrad_frames(d, ws2, T, N, wgrad->x, y, workspace, wgrad->dw, reserve, wgrad->max_blocks, wgrad->in_bound, 1,
                     b0, b1);
      }
      join_stream(ws2, s);  // the bias partials are written after the last flag
      wgrad_bias(d, ws2, T, N, wgrad->dw, reserve, 0);
      wgrad->done = true;
    }
    if (ver == 6) xch_release(s);
    tr.dump("bwd", s, grid.x, p.nwg, T, dirs, ver, ver == 6 ? (p.xpd ? 1 : 0) : p.xpd);
    if (dxl && !streamed && d.prec == kPrecBf16 && use_x3(NW * H)) {
      // bf16: dGates rows and W^T rows (columns of W) packed as bf16 (the
      // dGates rows written packed by the recurrence when pkd)
      const long G4 = (long)NW * H;
      const int KB = (int)((G4 + 63) / 64);
      const PackLay pl = pack_layout(d, T, N);
      __bf16 *Ap = pkd ? p.dxr : pk<__bf16>(workspace, d, T, N, pl.a), *Bp = pk<__bf16>(workspace, d, T, N, pl.b);
      {
        ProfSpan ps(s, "x3_pack");
        if (!pkd) bf16_pack_rows(s, DX, (long)dirs * G4, (int)TN, (int)G4, Ap, dirs, G4, TN * KB * 64);
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
    } else if (dxl && !streamed) {
      const bool x3 = use_x3(NW * H);
      const long G4 = (long)NW * H;
      const int KB = (int)((G4 + 31) / 32);
      const PackLay pl = pack_layout(d, T, N);
      _Float16 *Ap = pk<_Float16>(workspace, d, T, N, pl.a), *Bp = pk<_Float16>(workspace, d, T, N, pl.b);
      int *eA = pk<int>(workspace, d, T, N, pl.ea), *eB = pk<int>(workspace, d, T, N, pl.eb);
      unsigned *cm = pk<unsigned>(workspace, d, T, N, pl.cm);
      if (x3) {
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
        if (x3) {
          X3PArgs x;
          x.M = (int)TN; x.N = Din; x.KB = KB;
          x.A = Ap + (long)dir * TN * KB * 64; x.eA = eA + (long)dir * TN;
          x.B = Bp + (long)dir * Din * KB * 64; x.eB = eB + dir * Din;
          x.C = dxl; x.ldc = Din; x.beta = dir == 0 ? 0.f : 1.f;
          gemm_x3p(s, x);
        } else {
          GemmArgs g;
          g.transA = false; g.transB = false;
          g.M = (int)TN; g.N = Din; g.K = NW * H;
          g.A = DX + (long)dir * NW * H; g.lda = (long)dirs * NW * H;
          g.B = wl + dir * pls; g.ldb = Din;
          g.C = dxl; g.ldc = Din;
          g.beta = dir == 0 ? 0.f : 1.f;
          gemm_f32(s, g);
        }
      }
    }
    dcur = dxl;
  }
  return KRNN_OK;
}

// ---------------------------------------------------------------------------
// host: backward weights (accumulates into dw, like cudnnRNNBackwardWeights)
// ---------------------------------------------------------------------------
int rnn_backward_weights(const RnnDesc &d, hipStream_t s, int T, int N, const float *x,
                         const float *y, void *workspace, size_t ws_bytes, float *dw,
                         void *reserve, size_t res_bytes, int max_blocks, float in_bound, hipStream_t s2,
                         const void *in_cols, bool beside, const RnnPrepack *pre) {
  const RnnReserveLayout lay = rnn_reserve_layout(d, T, N);
  if (res_bytes < sizeof(float) * (size_t)lay.total) return KRNN_BAD_PARAM;
  if (ws_bytes < rnn_workspace_bytes(d, T, N)) return KRNN_BAD_PARAM;
  const int NW = d.nw(), H = d.H, dirs = d.dirs, G4 = NW * H;
  const long TN = (long)T * N;
  float *res = static_cast<float *>(reserve);
  float *ws = static_cast<float *>(workspace);
  for (int l = 0; l < d.layers; l++) {
    float *R0 = res + lay.per_layer * l;
    const float *in = l == 0 ? x : res + lay.per_layer * (l - 1) + lay.out;
    const float *out = (l == d.layers - 1) ? y : R0 + lay.out;
    const int Din = d.din(l);
    const long pl0 = d.lin_offset(l * dirs, 0, false);
    const long pls = d.pl_size(l);
    float *dwl = dw + pl0;
    float *E = R0 + lay.E;
    float *DX = d.mode == kGru ? R0 + lay.DX : E;
    const long ldg = (long)dirs * G4, ldy = (long)dirs * H;
    // dW_dir += DX_dir^T x
    GemmArgs g;
    g.transA = true; g.transB = false;
    g.M = G4; g.N = Din; g.K = (int)TN;
    g.A = DX; g.lda = ldg; g.B = in; g.ldb = Din;
    g.C = dwl; g.ldc = Din; g.beta = 1.f;
    g.batch = dirs; g.strideA = G4; g.strideB = 0; g.strideC = pls;
    g.split_k = gemm_pick_split(g.M, g.N, g.K, dirs);
    g.ws = ws;
    g.max_blocks = max_blocks;
    // flag words 1008..1009 of the workspace: dynamic tile counters (the
    // recurrences of this layer, which use the other flag words, are done)
    unsigned *fl = reinterpret_cast<unsigned *>(static_cast<char *>(workspace) + flags_offset(d, T, N));
    if (max_blocks > 0) g.tile_counter = reinterpret_cast<int *>(fl + 1008);
    // K = frames: large (also for a 40-dim input: 0.8 ms/step over fp32).
    // A bf16 backward that wrote its dGates packed (bf16_direct) left no fp32
    // rows: its packed operands are the only ones, however few the frames
    // (under 128 frames the fp32 GEMMs below read rows nobody had written)
    const bool x3 = use_x3((int)TN) || bf16_direct(d, 6);
    if (x3 && d.prec == kPrecBf16) {
      // bf16 weight GEMMs: the transposes packed along the frames as bf16
      const int KB = (int)((TN + 63) / 64);
      const PackLay pl = pack_layout(d, T, N);
      // the dGates transposes: written packed by the backward recurrence (bf16_direct)
      const bool pkd = bf16_direct(d, 6);
      // bf16_io: the forward wrote y^T packed (unshifted) and the backward
      // E^T shifted by one step; the input's columns may come packed from the
      // previous component's forward (in_cols)
      const bool io = bf16_io(d);
      const bool cols_in = l == 0 && in_cols != nullptr;
      __bf16 *DXt = pkd ? reinterpret_cast<__bf16 *>(R0 + lay.pkxt) : pk<__bf16>(workspace, d, T, N, pl.a);
      __bf16 *Xt = cols_in ? static_cast<__bf16 *>(const_cast<void *>(in_cols)) : pk<__bf16>(workspace, d, T, N, pl.b);
      __bf16 *Yt = io ? reinterpret_cast<__bf16 *>(R0 + lay.pkyc) : pk<__bf16>(workspace, d, T, N, pl.c);
      __bf16 *Et = (d.mode == kGru || io)
                       ? (pkd ? reinterpret_cast<__bf16 *>(R0 + lay.pket) : DXt + (long)dirs * G4 * KB * 64)
                       : DXt;
      {
        ProfSpan ps(s, "x3_pack_w");
        if (!pkd) {
          bf16_pack_cols(s, DX, ldg, (int)TN, (int)(dirs * G4), 0, DXt);
          if (d.mode == kGru) bf16_pack_cols(s, E, ldg, (int)TN, (int)(dirs * G4), 0, Et);
        }
        if (!cols_in) bf16_pack_cols(s, in, Din, (int)TN, Din, 0, Xt);
        if (T > 1 && !io)
          for (int dir = 0; dir < dirs; dir++)
            bf16_pack_cols(s, out + (long)dir * H, ldy, (int)TN, H, dir == 0 ? N : -N, Yt + (long)dir * H * KB * 64);
      }
      {
        X3PArgs x;
        x.bf16 = true;
        x.M = (int)G4; x.N = Din; x.KB = KB;
        x.A = reinterpret_cast<const _Float16 *>(DXt); x.sA = G4 * KB * 64;
        x.B = reinterpret_cast<const _Float16 *>(Xt);
        x.C = dwl; x.ldc = Din; x.beta = 1.f;
        x.batch = dirs; x.sC = pls;
        x.split_k = x3p_pick_split((int)G4, Din, KB, dirs); x.ws = ws;
        x.max_blocks = g.max_blocks; x.tile_counter = g.tile_counter;
        ProfSpan ps(s, "gemm_bwd_w");
        gemm_x3p(s, x);
      }
      if (T > 1) {
        X3PArgs x;
        x.bf16 = true;
        x.M = (int)G4; x.N = H; x.KB = KB;
        x.A = reinterpret_cast<const _Float16 *>(Et); x.sA = G4 * KB * 64;
        x.B = reinterpret_cast<const _Float16 *>(Yt); x.sB = (long)H * KB * 64;
        x.C = dwl + (d.lin_offset(l * dirs, NW, false) - pl0); x.ldc = H; x.beta = 1.f;
        x.batch = dirs; x.sC = pls;
        x.split_k = x3p_pick_split((int)G4, H, KB, dirs); x.ws = ws;
        x.max_blocks = max_blocks;
        if (max_blocks > 0) x.tile_counter = reinterpret_cast<int *>(fl + 1009);
        ProfSpan ps(s, "gemm_bwd_r");
        gemm_x3p(s, x);
      }
    }
    if (x3 && d.prec == kPrecBf16) {
    } else {
    const int KBt = (int)((TN + 31) / 32);
    const PackLay pl = pack_layout(d, T, N);
    // x^T and y^T packed by the forward (RnnPrepack::wgrad), else here
    const bool wpre = pre && pre->wdone && pre->wev && use_x3((int)TN) && d.layers == 1 && T > 1;
    _Float16 *DXt = pk<_Float16>(workspace, d, T, N, pl.a);
    _Float16 *Xt = pk<_Float16>(workspace, d, T, N, wpre ? pl.xt : pl.b);
    _Float16 *Yt = pk<_Float16>(workspace, d, T, N, wpre ? pl.yt : pl.c);
    _Float16 *Et = d.mode == kGru ? DXt + (long)dirs * G4 * KBt * 64 : DXt;
    int *eDX = pk<int>(workspace, d, T, N, pl.ea), *eX = pk<int>(workspace, d, T, N, wpre ? pl.ext : pl.eb);
    int *eY = pk<int>(workspace, d, T, N, wpre ? pl.eyt : pl.ec), *eE = d.mode == kGru ? pk<int>(workspace, d, T, N, pl.ed) : eDX;
    if (wpre) KCTC_HIP_CHECK(hipStreamWaitEvent(s, pre->wev, 0));
    unsigned *cm = pk<unsigned>(workspace, d, T, N, pl.cm);
    // two streams (s2, the bottom component's tail, where nothing else
    // overlaps): input^T and output^T are packed and dW runs on s2 while
    // dGates^T is packed and dR runs on s (separate split slabs, tile
    // counters and absmax scratch); s then waits for s2
    const unsigned *cme0 = pick6(d, N, false) ? pk<unsigned>(workspace, d, T, N, pl.cme) : nullptr;
    // (LSTM: dR's dGates^T is dW's, E == DX; the GRU's E^T pack stays on one stream)
    const bool two = s2 && x3 && cme0 && d.mode == kLstm && d.layers == 1 && T > 1 && env_int("KCTC_WGRAD_2S", 1);
    hipStream_t sx = two ? s2 : s;  // stream of the input / output packs and of dW
    hipEvent_t ev_dx = nullptr, ev_y = nullptr;
    if (two) {
      KCTC_HIP_CHECK(hipEventCreateWithFlags(&ev_dx, hipEventDisableTiming));
      KCTC_HIP_CHECK(hipEventCreateWithFlags(&ev_y, hipEventDisableTiming));
      join_stream(s2, s);
    }
    if (two) {
      ProfSpan ps(s, "x3_pack_w");
      x3p_pack_cols(s, DX, ldg, (int)TN, (int)(dirs * G4), 0, DXt, eDX, cme0, 0.f);
      KCTC_HIP_CHECK(hipEventRecord(ev_dx, s));
      const bool xb = l == 0 && in_bound > 0.f;
      // absmax scratch of its own: the GRU-only E^T exponent array (free for an LSTM)
      unsigned *cmx = reinterpret_cast<unsigned *>(pk<int>(workspace, d, T, N, pl.ed));
      if (!wpre) {
        if (!xb) absmax_f32(s2, in, Din, (int)TN, Din, nullptr, cmx);
        x3p_pack_cols(s2, in, Din, (int)TN, Din, 0, Xt, eX, cmx, xb ? in_bound : 0.f);
        for (int dir = 0; dir < dirs; dir++)
          x3p_pack_cols(s2, out + (long)dir * H, ldy, (int)TN, H, dir == 0 ? N : -N, Yt + (long)dir * H * KBt * 64,
                        eY + dir * H, nullptr, 1.f);
      }
      KCTC_HIP_CHECK(hipEventRecord(ev_y, s2));
      KCTC_HIP_CHECK(hipStreamWaitEvent(s2, ev_dx, 0));
      KCTC_HIP_CHECK(hipStreamWaitEvent(s, ev_y, 0));
    } else if (x3) {
      // the transposes, packed over the frames: dGates^T (per-gate exponents),
      // input^T (per-dim), and for dR the output shifted by one step per direction
      ProfSpan ps(s, "x3_pack_w");
      // beside a pinned recurrence: off its XCDs (x3p_pack_cols avoid)
      const unsigned *av = beside ? rnn_pinned_xcds() : nullptr;
      const int nx = std::max(1, rnn_usable_cus() / kCusPerXcd);
      // their item counters: flag words 1010..1014 (this component's
      // recurrences, which use the flag words, are done)
      int *pc = reinterpret_cast<int *>(fl + 1010);
      if (av) KCTC_HIP_CHECK(hipMemsetAsync(pc, 0, sizeof(int) * 5, s));
      // the v6 backward recurrence leaves the dGates column maxima behind
      const unsigned *cme = cme0;
      if (!cme) absmax_f32(s, DX, ldg, (int)TN, (int)(dirs * G4), nullptr, cm);
      x3p_pack_cols(s, DX, ldg, (int)TN, (int)(dirs * G4), 0, DXt, eDX, cme ? cme : cm, 0.f, 1, 0, 0, 0, 0, av, nx,
                    pc);
      if (d.mode == kGru) {
        if (!cme) absmax_f32(s, E, ldg, (int)TN, (int)(dirs * G4), nullptr, cm);
        x3p_pack_cols(s, E, ldg, (int)TN, (int)(dirs * G4), 0, Et, eE, cme ? cme + dirs * G4 : cm, 0.f, 1, 0, 0, 0,
                      0, av, nx, pc + 1);
      }
      const bool xb = (l > 0 && bounded_out(d)) || (l == 0 && in_bound > 0.f);
      if (!xb && !wpre) absmax_f32(s, in, Din, (int)TN, Din, nullptr, cm);
      if (!wpre)
        x3p_pack_cols(s, in, Din, (int)TN, Din, 0, Xt, eX, cm, xb ? (l > 0 ? 1.f : in_bound) : 0.f, 1, 0, 0, 0, 0,
                      av, nx, pc + 2);
      if (T > 1 && !wpre) {
        if (!bounded_out(d)) absmax_f32(s, out, ldy, (int)TN, (int)ldy, nullptr, cm);
        for (int dir = 0; dir < dirs; dir++)
          x3p_pack_cols(s, out + (long)dir * H, ldy, (int)TN, H, dir == 0 ? N : -N, Yt + (long)dir * H * KBt * 64,
                        eY + dir * H, bounded_out(d) ? nullptr : cm + dir * H, bounded_out(d) ? 1.f : 0.f, 1, 0, 0,
                        0, 0, av, nx, pc + 3 + dir);
      }
    }
    // beside another component's pinned backward recurrence: dW and dR as
    // one launch on the CUs it leaves (gemm_x3p_pair; configs[1]: the side
    // stream fell one GEMM per layer behind, 4 ms of weight GEMMs after the
    // last recurrence)
    const bool pair = beside && x3 && !two && T > 1 && x3p_use_256((int)G4, Din) && x3p_use_256((int)G4, H) &&
                      max_blocks > 0;
    X3PArgs xw;
    if (x3) {
      X3PArgs &x = xw;
      x.M = (int)G4; x.N = Din; x.KB = KBt;
      x.A = DXt; x.eA = eDX; x.sA = G4 * KBt * 64; x.seA = G4;
      x.B = Xt; x.eB = eX;
      x.C = dwl; x.ldc = Din; x.beta = 1.f;
      x.batch = dirs; x.sC = pls;
      x.split_k = x3p_pick_split((int)G4, Din, KBt, dirs);
      // concurrent with dR: its own split slab past dR's (none when dR is not
      // split: drec_split_floats reserves a dR slab only for a split > 1)
      const long sR = x3p_pick_split((int)G4, H, KBt, dirs);
      x.ws = (two || pair) && sR > 1 ? ws + al64(sR * dirs * G4 * H) : ws;
      x.max_blocks = g.max_blocks; x.tile_counter = g.tile_counter;
      if (pair) {
        x.max_blocks = 192;
        x.avoid_word = rnn_pinned_xcds();
        x.avoid_xcds = std::max(1, rnn_usable_cus() / kCusPerXcd);
      } else {
        ProfSpan ps(sx, "gemm_bwd_w");
        gemm_x3p(sx, x);
      }
    } else {
      ProfSpan ps(s, "gemm_bwd_w");
      gemm_f32(s, g);
    }
    // dR_dir += E_dir(shifted)^T h_prev:  fwd pairs rows t>=1 with y rows t-1,
    // bwd pairs rows t<=T-2 with y rows t+1 (column half H..2H-1)
    if (T > 1) {
      GemmArgs r;
      r.transA = true; r.transB = false;
      r.M = G4; r.N = H; r.K = (int)((long)(T - 1) * N);
      r.A = E + (long)N * ldg; r.lda = ldg;
      r.B = out; r.ldb = ldy;
      r.C = dwl + (d.lin_offset(l * dirs, NW, false) - pl0); r.ldc = H; r.beta = 1.f;
      r.batch = dirs;
      r.strideA = (long)G4 - (long)N * ldg;        // dir 1: E + G4 (rows 0..T-2)
      r.strideB = (long)N * ldy + H;               // dir 1: y rows 1..T-1, cols H..
      r.strideC = pls;
      r.split_k = gemm_pick_split(r.M, r.N, r.K, dirs);
      r.ws = ws;
      r.max_blocks = max_blocks;
      if (max_blocks > 0) r.tile_counter = reinterpret_cast<int *>(fl + 1009);
      ProfSpan ps(s, "gemm_bwd_r");
      if (x3) {
        // all frames: the shifted-out ones are zero in the packed output
        X3PArgs x;
        x.M = (int)G4; x.N = H; x.KB = KBt;
        x.A = Et; x.eA = eE; x.sA = G4 * KBt * 64; x.seA = G4;
        x.B = Yt; x.eB = eY; x.sB = (long)H * KBt * 64; x.seB = H;
        x.C = r.C; x.ldc = H; x.beta = 1.f;
        x.batch = dirs; x.sC = pls;
        x.split_k = x3p_pick_split((int)G4, H, KBt, dirs); x.ws = ws;
        x.max_blocks = max_blocks; x.tile_counter = r.tile_counter;
        if (pair) gemm_x3p_pair(s, xw, x);  // xw's tile counter, block count and avoid word
        else gemm_x3p(s, x);
      } else {
        gemm_f32(s, r);
      }
    }
    if (two) {
      join_stream(s, s2);
      (void)hipEventDestroy(ev_dx);
      (void)hipEventDestroy(ev_y);
    }
    }  // x3 / fp32 weight GEMMs
    // biases: dbW += sum dGx, dbR += sum dGh (partials from the recurrence)
    const long bW = d.lin_offset(l * dirs, 0, true) - pl0;
    const long bR = d.lin_offset(l * dirs, NW, true) - pl0;
    // (v6: one partial per row group, [group][dir][2][G], added in group order)
    const V6Cfg c6b = pick6(d, N, false);
    const int rg = c6b ? c6b.rg : 1;
    for (int gi = 0; gi < rg; gi++)
      for (int dir = 0; dir < dirs; dir++) {
        const float *part = R0 + lay.bias + ((long)gi * dirs + dir) * 2 * G4;
        clip_sgd_update(s, dwl + dir * pls + bW, part, G4, 1.f, 0.f);
        clip_sgd_update(s, dwl + dir * pls + bR, part + G4, G4, 1.f, 0.f);
      }
  }
  return KRNN_OK;
}

}  // namespace kctc
