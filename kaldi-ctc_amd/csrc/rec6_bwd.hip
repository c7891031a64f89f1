// rec6_bwd.hip -- rnn_bwd_rec6, the v6 backward-data recurrence, and its half
// of the kernel lookup.  Host side and protocol: rnn.hip.
#include "rec_common.h"

namespace kctc {
namespace {

// ---------------------------------------------------------------------------
// v6 backward: reduce-scatter hand-off, split-fp16 MFMA
// ---------------------------------------------------------------------------
// WG (dir, g) owns units u0..u0+U-1 and the K = nW*U rows of R that feed those
// units' gates.  Per step it
//   (1) sums the partial dh of its units from every producer WG of its
//       direction (published the step before; fixed summation order),
//   (2) does the pointwise cell backward of its (n, unit) elements (one per
//       thread) -> dGates [N x K],
//   (3) multiplies dGates [16 x K] by its R rows [K x H] on the matrix cores,
//       every wave owning H/4 output columns (no cross-wave reduction), and
//   (4) publishes that partial dh of ALL H units, fp32, in the MFMA C-fragment
//       layout [producer][col tile][lane][4] (1 KB per 16 x 16 tile).
// Per WG and step 32 KB are read and 32 KB written (BLSTM-512, N=16) instead of
// the 128 KB dGates all-gather of the generic backward (rec_generic.hip).
//
// Split-fp16 products ("fp16x3"): both operands are scaled by powers of two
// (R slice: one exponent per WG, from its max |R|; dGates: one exponent per
// row, from the row's max over the WG's K columns) so the largest magnitude
// lands in [2^13, 2^14), and split as x = hi + lo with hi = fp16(x),
// lo = fp16(x - hi).  acc += hi_a hi_b + hi_a lo_b + lo_a hi_b on
// v_mfma_f32_16x16x32_f16 (products exact, fp32 accumulation), then the exact
// power-of-two unscale.  Each operand keeps 22 significant bits relative to
// its row / slice maximum; the dropped lo*lo term is 2^-22 of it -- the same
// order as fp32 rounding of the accumulated terms.  5.3x fewer MFMA cycles
// than v_mfma_f32_16x16x4_f32 for the same product.
//
// R lives in registers for the whole launch (the B fragments of the wave's
// H/64 column tiles, hi and lo); dGates goes through a 4.5 KB LDS image.
// Hand-off as rec_generic.hip (sc1 payload stores, vmcnt(0), barrier, sc1 epoch flag;
// sc1 loads) into a per-step image that is never rewritten within a launch.
// Generalisation (row groups, wide workgroups, bf16): the N sequences are
// split into RG = ceil(N / 16) groups of 16 rows, each an independent
// recurrence on its own dirs x NWG workgroups, flag lines and exchange images
// (block b -> direction b % dirs, workgroup (b / dirs) % NWG, group
// b / (dirs NWG)); a workgroup of NTH = 256 or 512 threads owns U = 8, 16 or
// 32 units (one (row, unit) element per thread, NTH / 64 waves each owning
// H / (16 NTH / 64) output column tiles).  P = kPrecBf16 multiplies bf16
// dGates by a bf16 R slice instead of the split-fp16 pair (one MFMA per
// block, no scaling; partial dh stay fp32).
// Stacked backward: the partial-dh stores are pipelined behind the next tile's
// MFMAs, and the hand-off loads run on half the waves with every lane live
// (HO4).  bf16 backward: the previous step's dGates stores go under the
// hand-off loads.
template <int MODE, int U, int H, int NTH, int P>
__global__ __launch_bounds__(NTH, 1) void rnn_bwd_rec6(RecParams p) {
  REC_TRACE_INIT;
  constexpr int NW = MODE == kLstm ? 4 : 3;
  constexpr int NWV = NTH / 64;
  constexpr int K = NW * U, KB = (K + 31) / 32, AP = KB * 32 + 8;  // A image row pitch (halves)
  constexpr int CTW = H / (16 * NWV), CTT = H / 16, NWG = H / U;
  static_assert(CTW * 16 * NWV == H, "output column tiles per wave");
  static_assert(16 * U <= NTH, "one (row, unit) element per thread");
  constexpr int POS = 4 * U;       // 16-B chunks of the own column tiles per producer
  constexpr int NGRP = NTH / POS;  // producer groups
  constexpr int PER = NWG / NGRP;  // producers summed per group
  static_assert(NWG % NGRP == 0, "producer groups");
  constexpr bool BF = P == kPrecBf16;
  constexpr bool STK = P == kPrecX3S;  // dGates hi / lo stacked in one 16-row A image (groups of <= 8 rows)
  // split-fp16: the cell's coefficients before the hand-off (see kc below);
  // bf16 (configs[4], every wave an element wave) measured faster with the
  // whole pointwise backward in the cell (3.65 vs 3.46 us/step)
  constexpr bool PRE = !BF;
  // stacked: the operands come through LDS from waves 6 and 7 (IOA, io_fetch
  // below), the dGates rows leave through the estg stage with or without a
  // streaming consumer (RST), and wave 4 stores the aggregated epoch (GF4)
  constexpr bool IOA = STK, RST = STK, GF4 = STK;
  using AT = typename std::conditional<BF, __bf16, _Float16>::type;
  using AV = typename std::conditional<BF, bf16x8, halfx8>::type;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ int bad_lds, loc_lds;
  __shared__ int rowexp[16];
  __shared__ float wmax[NWV];
  // xpd = 1: XCD-slot mapping (block b -> direction b & 7, so a direction's 32
  // workgroups share one XCD under round-robin dispatch; checked by probe6;
  // one row group only); else block b -> (group, workgroup, direction)
  const int dirs = p.dirs;
  const int d = p.xpd ? (blockIdx.x & 7) % dirs : blockIdx.x % dirs;
  const int g = p.xpd ? (blockIdx.x >> 3) : (blockIdx.x / dirs) % NWG;
  const int grp = p.xpd ? (blockIdx.x & 7) / dirs : blockIdx.x / (dirs * NWG);
  if (d >= dirs || g >= NWG || grp >= p.rg) return;
  // resident: counted for the exchange's residency gate (rnn_comm_gate) and
  // in the launch's own word for the side launches beside it (beside_recurrence)
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(p.flags + kResWord, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p.reg) {
      __hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(p.reg + 4), 1ull, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
      if (p.xpd) __hip_atomic_fetch_or(p.reg + 2, 1u << xcc_id(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // rnn_pinned_xcds
    }
  }
  // rows n0 .. nend-1 of the batch (p.gs <= 16 of the 16 MFMA rows)
  const int N = p.N, T = p.T, n0 = grp * p.gs, nend = min(N, n0 + p.gs);
  const int u0 = g * U, ct_own = u0 >> 4, fr0 = u0 & 15;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const long ldy = (long)dirs * H, ldg = (long)dirs * NW * H;
  // floats per producer block (16 x H) + 256 B, so that the 1-KB chunks a
  // consumer reads from consecutive producers fall in different L2 channels
  // bf16 mode (p.bfpart): the partials travel as bf16 (8 B per lane and tile,
  // summed in fp32 by the consumer), half the bytes of the fp32 images
  const bool bfp = BF && p.bfpart;
  const long PSTR = bfp ? (long)CTT * 64 * 2 + 64 : (long)CTT * 64 * 4 + 64;
  const int LW = bfp ? 2 : 4;  // floats-worth per lane and tile
  const long xgrp = (long)dirs * NWG * PSTR;  // one row group's images of a step
  const long xstep = xgrp * p.rg;
  AT *Ahi = reinterpret_cast<AT *>(smem);  // [16][AP]
  AT *Alo = Ahi + 16 * AP;                 // x3 only
  float *red = reinterpret_cast<float *>(Alo + (BF ? 0 : 16 * AP));  // [NGRP][POS][4]
  // streamed consumer: this step's dGates tile [16][NW * U] (DX for GRU), then
  // written through with 16-B stores after the step's signal
  float *estg = red + (NTH * 4 > 2 * 16 * U * NW ? NTH * 4 : 2 * 16 * U * NW);
  const float *Wd = p.w + d * p.pl_stride;
  const float *R = Wd + p.r_off;
  if (tid == 0) bad_lds = 0;
  for (int i = tid; i < (BF ? 16 : 32) * AP; i += NTH) Ahi[i] = (AT)0.f;  // the image(s), padding included
  // ---- R slice -> B fragments in registers (x3: scaled hi/lo; bf16: as is) ----
  // K order of the dGates operand: split-fp16 paths unit-major (k = u NW + q:
  // an element's NW gates are adjacent halves, one 8-B LDS write per part),
  // bf16 gate-major (k = q U + u)
  constexpr bool KUM = !BF;
  auto rval = [&](int kk, int col) -> float {
    if (kk >= K) return 0.f;
    const int q = KUM ? kk % NW : kk / U, u = KUM ? kk / NW : kk - (kk / U) * U;
    return R[(long)(q * H + u0 + u) * H + col];
  };
  int sB = 0;
  if constexpr (!BF) {
    float mx = 0.f;
#pragma unroll
    for (int c = 0; c < CTW; c++)
#pragma unroll
      for (int kb = 0; kb < KB; kb++)
#pragma unroll
        for (int j = 0; j < 8; j++) mx = fmaxf(mx, fabsf(rval(kb * 32 + fq * 8 + j, (w * CTW + c) * 16 + fr)));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if (lane == 0) wmax[w] = mx;
    __syncthreads();
    float m4 = wmax[0];
#pragma unroll
    for (int i = 1; i < NWV; i++) m4 = fmaxf(m4, wmax[i]);
    sB = split_exp(m4);
  }
  AV bhi[CTW][KB], blo[BF ? 1 : CTW][BF ? 1 : KB];
  if constexpr (!BF) {
#pragma unroll
    for (int c = 0; c < CTW; c++)
#pragma unroll
      for (int kb = 0; kb < KB; kb++)
#pragma unroll
        for (int j = 0; j < 8; j++) {
          _Float16 h, l;
          split16(ldexpf(rval(kb * 32 + fq * 8 + j, (w * CTW + c) * 16 + fr), sB), h, l);
          bhi[c][kb][j] = h;
          blo[c][kb][j] = l;
        }
  }
  // bf16: filled after the start-up wait (probe6) below -- filled here, hipcc
  // sank the conversions past that wait loop with all 8 x KB x CTW fp32
  // values live and spilled the 512-thread GRU kernel to scratch (before the
  // step loop, but a kernel with scratch must run alone: rec6_scratch_free)
  // ---- per-element state: thread tid <-> (row n0 + en, unit u0 + eu) ----
  // STK: a group has at most 8 rows, so the element threads are whole waves
  // (tid < 8 U) and the others run no coefficients, reduction reads, cell or
  // bookkeeping; rows 8..15 of the [16][U] reductions behind the loop come
  // from the has_r threads, as zeros
  const bool has_r = tid < 16 * U;
  const bool has_e = tid < (STK ? 8 : 16) * U;
  // IOA (stacked): the last 8 U threads, waves 6 and 7, are the element
  // threads' twins -- thread tid of them fetches the operands of element
  // tid - (NTH - 8 U) into the LDS stage (io_fetch below) and does nothing
  // else of an element's work
  const bool io_lane = IOA && tid >= NTH - 8 * U;
  const bool io_wave = IOA && __builtin_amdgcn_readfirstlane(tid >> 6) >= NWV - 8 * U / 64;
  const int etid = io_lane ? tid - (NTH - 8 * U) : tid;
  const int en = etid / U, eu = etid - en * U;
  const int n = n0 + en;
  const bool live = has_e && n < nend;
  float carry = 0.f, bsx[NW], bsh[NW], dxk[NW], eg[NW], cg[NW], ng[NW], cmx[NW], cme[NW];
  float cdy = 0.f, ca = 0.f, cap_ld = 0.f, ndy = 0.f, na = 0.f, nap = 0.f;
  // The cell's coefficients -- everything of the pointwise backward that does
  // not depend on the hand-off -- computed from the step's forward values
  // after the previous step's publish (while the other producers' epochs are
  // on their way), so that the cell after the hand-off is a few FMAs:
  //   LSTM: dc = dh kc[0] + carry, dG_q = dc kc[1+q] (q < 3), dG_3 = dh kc[4], carry = dc kc[5]
  //   GRU : dh += carry, dX_q = dh kc[q], dE_2 = dh kc[3], carry = dh kc[4]
  float kc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  auto coef = [&](int kk, bool first = false) {  // kk: the forward-order step of c*
    // (STK: the first frame's previous state is zeroed here, not by the prefetch)
    const float cap = (!STK || kk > 0) ? cap_ld : 0.f;
    // (STK: the fused multiply-adds spelled out, as they were contracted
    // before the two-ahead prefetch -- all of them, but for the LSTM's
    // 1 - g^2 of the first step (the copy in front of the loop), which had two
    // roundings and keeps them; left to the compiler, which of them fuse
    // depends on the code around, and with it the last bit of every result)
    auto omsq = [](float x) { return STK ? __builtin_fmaf(-x, x, 1.f) : 1.f - x * x; };
    auto omsq2 = [](float x) {
      float sq = x * x;
      asm volatile("" : "+v"(sq));
      return 1.f - sq;
    };
    if (MODE == kLstm) {
      const float ig = cg[0], fg = cg[1], gg = cg[2], og = cg[3];
      const float tc = STK ? __builtin_fmaf(2.f, fsigm(2.f * ca), -1.f) : ftanh(ca);
      kc[0] = og * omsq(tc);
      kc[1] = gg * ig * (1.f - ig);
      kc[2] = cap * fg * (1.f - fg);
      kc[3] = ig * ((STK && first) ? omsq2(gg) : omsq(gg));
      kc[4] = tc * og * (1.f - og);
      kc[5] = fg;
    } else {
      const float r = cg[0], z = cg[1], nn = cg[2];
      const float kn = (1.f - z) * omsq(nn);
      kc[0] = kn * ca * r * (1.f - r);
      kc[1] = (cap - nn) * z * (1.f - z);
      kc[2] = kn;
      kc[3] = kn * r;
      kc[4] = z;
    }
  };
  // bias and column-maximum bookkeeping of the step's dGates, and their LDS
  // stage for the next step's row writes
  auto book = [&]() {
#pragma unroll
    for (int q = 0; q < NW; q++) {
      bsx[q] += (MODE == kGru) ? dxk[q] : eg[q];
      if (MODE == kGru) bsh[q] += eg[q];
      if (live) {  // column maxima for the weight GEMMs' packed transposes
        cmx[q] = fmaxf(cmx[q], fabsf(MODE == kGru ? dxk[q] : eg[q]));
        if (MODE == kGru) cme[q] = fmaxf(cme[q], fabsf(eg[q]));
      }
    }
    if (RST || p.e_sc1 || (BF && p.dxt != nullptr)) {
#pragma unroll
      for (int q = 0; q < NW; q++) estg[en * NW * U + q * U + eu] = MODE == kGru ? dxk[q] : eg[q];
      if (MODE == kGru && BF && p.dxt != nullptr) {
#pragma unroll
        for (int q = 0; q < NW; q++) estg[16 * NW * U + en * NW * U + q * U + eu] = eg[q];
      }
    }
  };
#pragma unroll
  for (int q = 0; q < NW; q++) bsx[q] = bsh[q] = dxk[q] = eg[q] = cg[q] = ng[q] = cmx[q] = cme[q] = 0.f;
  // this element's operand columns as per-lane pointers, opaque to the
  // compiler: they stay in VGPRs and the kernel-argument bases die here
  // (the loop's scalar registers spill otherwise)
  // They start at the first step's time (forward-order step T - 1) and move
  // one step image per prefetch / row store (the loop's time moves by tstep
  // frames a step): no per-step index arithmetic.  The laundering leaves
  // generic pointers (FLAT loads, which count in lgkmcnt too, so that every
  // LDS wait before a barrier covered the HBM loads): cast back to global
  typedef const float __attribute__((address_space(1))) *gcfp;
  typedef float __attribute__((address_space(1))) *gfp;
  const int t_first = d == 0 ? T - 1 : 0;
  const long ystep = (d == 0 ? -1 : 1) * (long)N * ldy, gstep = (d == 0 ? -1 : 1) * (long)N * ldg;
  // (a fetching twin of a dead row reads a live row's operands: every lane of
  // the IO waves issues every load, so that their vmcnt counts are exact)
  const int nld = io_lane ? max(n0, min(n, nend - 1)) : n;
  const long yel = ((long)t_first * N + nld) * ldy + (long)d * H + u0 + eu;
  const long gel = ((long)t_first * N + nld) * ldg + (long)d * NW * H + u0 + eu;
  const float *dy_e = p.dy + yel;
  const float *g_e = p.G + gel;
  const float *aux_e = p.aux + yel;
  const float *prv_e = (MODE == kLstm ? p.aux : p.y) + yel + ystep;  // the step before, in forward order
  float *e_e = p.E + gel;
  float *dx_e = (MODE == kGru ? p.DX : p.E) + gel;
  asm volatile("" : "+v"(dy_e), "+v"(g_e), "+v"(aux_e), "+v"(prv_e), "+v"(e_e), "+v"(dx_e));
  gcfp dy_p = (gcfp)dy_e, g_p = (gcfp)g_e, aux_p = (gcfp)aux_e, prv_p = (gcfp)prv_e;
  gfp e_p = (gfp)e_e, dx_p = (gfp)dx_e;
  auto prefetch = [&](int k) {  // operands of forward-order step k (T - 1, T - 2, ... in turn) into n*
    if (live) {
      ndy = *dy_p;
#pragma unroll
      for (int q = 0; q < NW; q++) ng[q] = g_p[q * H];
      na = *aux_p;
      if constexpr (STK) {
        // always loaded (first frame: a valid address, the value dropped by
        // coef()): a conditional load here tied nap to a zero in a register
        // pair and put a vmcnt(0) behind the loads
        const gcfp pp = k > 0 ? prv_p : aux_p;
        nap = *pp;
      } else {
        nap = k > 0 ? *prv_p : 0.f;
      }
    }
    dy_p += ystep; g_p += gstep; aux_p += ystep; prv_p += ystep;
  };
  // n* -> c*, where coef() and the cell read.  (STK: in front of the loop
  // only, for step 0; from step 1 on the element waves read c* from the LDS
  // slot the IO waves filled and issue no global load in the step loop)
  // (xdy, the stage dy had when the operands ran two steps ahead, has no
  // reader left; without the copy the compiler orders some instructions of the
  // plain split-fp16 kernels differently, and those stay the parent's to the letter)
  float xdy = 0.f;
  auto rotate = [&]() {
    xdy = cdy;
    cdy = ndy; ca = na; cap_ld = nap;
#pragma unroll
    for (int q = 0; q < NW; q++) cg[q] = ng[q];
    if constexpr (STK) {
      // one register each (as pairs, a half copied behind the prefetch's
      // loads put a vmcnt(0) there)
      asm volatile("" : "+v"(cdy), "+v"(ca), "+v"(cap_ld));
#pragma unroll
      for (int q = 0; q < NW; q++) asm volatile("" : "+v"(cg[q]));
    }
  };
  // IOA: the operand stage, a ring of three slots [NOP][8 U] floats behind
  // estg -- slot j % 3 holds the operands of step j (dy, the NW gates, c / the
  // GRU's aux, the previous state), element e at [op][e].  An IO wave fills
  // its 64 elements of an operand with one LDS-DMA (no register, no LDS write
  // instruction; inline asm, invisible to the compiler's wait counts, see
  // dma_lds_dword).  The pointers stay on the last step once there (io_j):
  // the fetches past the end load it again into a slot nobody reads, so that
  // the wave's queue has the same shape at every step.
  constexpr int NOP = NW + 3, OSL = NOP * 8 * U;  // operands; floats per slot
  float *ostg = estg + 16 * NW * U;
  static_assert(!IOA || (2 * 16 * AP * 2 + (NTH * 4 > 2 * 16 * U * NW ? NTH * 4 : 2 * 16 * U * NW) * 4 + 16 * NW * U * 4 +
                         3 * OSL * 4 <= 96 * 1024), "the operand stage fits the launch's LDS (bwd6_lds_bytes: >= 96 KB)");
  int io_j = 0;  // the step the IO lanes' pointers stand on
  auto io_fetch = [&](int slot) {
    const unsigned dst = __builtin_amdgcn_readfirstlane(
        (unsigned)reinterpret_cast<uintptr_t>(ostg + slot * OSL + (w - (NWV - 8 * U / 64)) * 64));
    dma_lds_dword((const float *)dy_p, dst);
#pragma unroll
    for (int q = 0; q < NW; q++) dma_lds_dword((const float *)(g_p + q * H), dst + (1 + q) * 8 * U * 4);
    dma_lds_dword((const float *)aux_p, dst + (1 + NW) * 8 * U * 4);
    // (the first frame's previous state: a valid address, the value dropped by coef())
    dma_lds_dword((const float *)(io_j < T - 1 ? prv_p : aux_p), dst + (2 + NW) * 8 * U * 4);
    if (io_j < T - 1) {
      dy_p += ystep; g_p += gstep; aux_p += ystep; prv_p += ystep;
      io_j++;
    }
  };
  // what an IO wave leaves in flight in front of a step's first barrier: the
  // fetch and the 4 partial-dh stores of the step before (see the loop)
  auto io_wait = [&]() {
    if constexpr (NOP == 7) asm volatile("s_waitcnt vmcnt(11)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
  };
  static_assert(!IOA || CTW == 4, "an IO wave's 4 partial-dh stores a step");
  // bf16 packed operands (p.dxt): the step's DX tile is staged in estg and the
  // GRU's E tile in estg2 during the cell phase; the next step writes them as
  // 16-B bf16 chunks (DX rows; DX^T and E^T columns of 8 frames)
  float *estg2 = estg + 16 * NW * U;
  const bool pk = BF && p.dxt != nullptr;
  auto pk_store = [&](int tt) {
    if constexpr (BF) {
      constexpr int RCH = NW * U / 8;  // 16-B row chunks per row
      const long TNl = (long)T * N, G4 = (long)NW * H;
      const long f0 = (long)tt * N + n0;
      // DX rows: thread -> (row, chunk)
      for (int i = tid; i < 16 * RCH; i += NTH) {
        const int rn = i / RCH, ch = i - rn * RCH, q = (ch * 8) / U, u = (ch * 8) % U;
        if (n0 + rn >= nend) continue;
        bf16x8 v;
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = (__bf16)estg[rn * NW * U + q * U + u + j];
        *reinterpret_cast<bf16x8 *>(p.dxr + ((long)d * TNl + f0 + rn) * G4 + q * H + u0 + u) = v;
      }
      // DX^T (and E^T) columns: thread -> (column, 8-frame half); aligned 16-B
      // chunks when the 8 frames are whole, else per frame.  E^T shifted
      // (eshift): frames of step 0 (direction 0) / T - 1 (direction 1) drop out
      const bool vec8 = (N % 8 == 0) && (n0 % 8 == 0);
      const int narr = (MODE == kGru || p.eshift) ? 2 : 1;
      const long esh = p.eshift ? (d == 0 ? -(long)N : (long)N) : 0;
      const bool edrop = p.eshift && (d == 0 ? tt == 0 : tt == T - 1);
      for (int i = tid; i < narr * NW * U * 2; i += NTH) {
        const int which = i / (NW * U * 2), rem = i - which * NW * U * 2, col = rem >> 1, half = rem & 1;
        if (which && edrop) continue;
        const float *src = (which && MODE == kGru) ? estg2 : estg;
        __bf16 *dst = (which ? p.et : p.dxt) + ((long)d * G4 + (col / U) * H + u0 + col % U) * p.kbt64 + f0 + half * 8 +
                      (which ? esh : 0);
        const int r0 = half * 8;
        if (vec8 && n0 + r0 + 8 <= nend) {
          bf16x8 v;
#pragma unroll
          for (int j = 0; j < 8; j++) v[j] = (__bf16)src[(r0 + j) * NW * U + col];
          *reinterpret_cast<bf16x8 *>(dst) = v;
        } else {
          for (int j = 0; j < 8; j++)
            if (n0 + r0 + j < nend) dst[j] = (__bf16)src[(r0 + j) * NW * U + col];
        }
      }
    }
  };
  // row-major dGates of step t (E; GRU also DX): the loop's steps in turn,
  // e_p / dx_p move on by one step image a call
  auto e_store = [&](int t) {
    const gfp ep = e_p, dp = dx_p;
    e_p += gstep; dx_p += gstep;
    if (pk) {
      pk_store(t);
      return;
    }
    if (!live) return;
    if (RST || p.e_sc1) {  // DX (== E for LSTM) went out through estg already
      if (MODE == kGru) {
#pragma unroll
        for (int q = 0; q < NW; q++) ep[q * H] = eg[q];
      }
      return;
    }
#pragma unroll
    for (int q = 0; q < NW; q++) ep[q * H] = eg[q];
    if (MODE == kGru) {
#pragma unroll
      for (int q = 0; q < NW; q++) dp[q * H] = dxk[q];
    }
  };
  // consumer chunk of this thread: position pos (of the own column tiles'
  // C-fragment chunks) of producers pg, pg + NGRP, ...
  // HO4 (stacked, 32 live chunks a tile): the lower half of the waves load,
  // half a wave per producer -- lanes 0..31 the 512-B run of producer pg,
  // lanes 32..63 that of pg + 1 -- the same four producers in the same order
  // as the live half of wave pg did; the upper half of the waves load nothing
  constexpr bool HO4 = STK;
  static_assert(!HO4 || (POS == 64 && 8 * U <= NTH / 2), "32 live chunks a tile; the element waves load");
  const bool ho_wave = !HO4 || __builtin_amdgcn_readfirstlane(w) < NWV / 2;
  // (a wave that does not load: its pg, past the producer groups, is never used)
  const int pos = HO4 ? tid % (POS / 2) : tid % POS, pg = HO4 ? tid / (POS / 2) : tid / POS;
  const int pln = U >= 16 ? pos : (pos >> 3) * 16 + fr0 + (pos & 7);
  const long coff = (long)grp * xgrp + (long)d * NWG * PSTR + ((long)ct_own * 64 + pln) * LW + (long)pg * PSTR;
  // a C-fragment lane holds rows 4 (lane / 16) .. +3 of the group: quads past N
  // are neither stored nor loaded (a group of fewer than 16 sequences moves
  // only its own rows).  STK (transposed, U = 16): chunk j = 8 (unit / 4) +
  // row of a tile holds units 4 (j / 8) .. +3 of row j % 8, chunks 32..63 unused
  const bool crow_live = STK ? (pln < 32 && n0 + (pln & 7) < nend) : n0 + 4 * ((pln & 63) >> 4) < nend;
  const bool prow_live = STK ? (fr < 8 && n0 + fr < nend) : n0 + 4 * fq < nend;
  // where element (en, eu) finds its sum: own tile eu / 16, lane (en / 4) * 16
  // + (eu % 16) (U = 8: compacted to 8 per row quad), register en % 4
  const int epos = STK ? (eu >> 2) * 8 + en : (eu >> 4) * 64 + (en >> 2) * (U < 16 ? U : 16) + (eu & 15);
  const int ereg = STK ? (eu & 3) : (en & 3);
  prefetch(T - 1);
  rotate();
  if constexpr (IOA) {
    // step 0's operands came directly (above); those of steps 1 and 2 are in
    // their slots before the loop (the first read of a slot follows step 0's
    // two barriers), so that every wait in the loop finds the same queue
    if (io_wave) {
      if (T > 1) {
        io_j = 1;  // (prefetch() moved the pointers on)
      } else {
        dy_p -= ystep; g_p -= gstep; aux_p -= ystep; prv_p -= ystep;
      }
      io_fetch(1);
      io_fetch(2);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  if constexpr (PRE) {
    if (!STK || has_e) coef(T - 1, true);
  }
  int bad = 0;
  unsigned *myflag = flag6(p, grp, d, g, NWG);
  // XCD-slot launches keep the hand-off in the XCD's L2 (plain flag stores
  // other XCDs do not see).  For the streamed dx GEMM running on the other
  // XCDs, workgroup 0 of each (row group, direction) publishes ONE aggregated
  // sc1 epoch (agg_flag6): after the first barrier of step ks it has seen every
  // producer's epoch ks + 1, whose signals drained their rows of step ks - 2,
  // so it stores ks + 1 ("rows of step k complete at epoch k + 3").  One line
  // per direction instead of 32 for up to ~100 polling GEMM blocks.
  unsigned *gflag = (p.xpd && p.e_sc1 && g == 0) ? agg_flag6(p, grp, d) : nullptr;
  // and where it runs, for the streamed GEMM's blocks (on_pinned_xcd)
  // (before any wait on another workgroup: a residency gate block on this XCD
  // leaves on it, rnn_resident_gate)
  if (p.xpd && tid == 0) atomicOr(p.flags + kXcdWord, 1u << xcc_id());
  if (tid == 0) loc_lds = 0;
  const int local = (p.xpd && p.allow_local) ? probe6(p, grp, d, g, NWG, bad, &bad_lds, &loc_lds) : 0;
  if constexpr (BF) {
    auto fill = [&]() {
#pragma unroll
      for (int c = 0; c < CTW; c++)
#pragma unroll
        for (int kb = 0; kb < KB; kb++)
#pragma unroll
          for (int j = 0; j < 8; j++) bhi[c][kb][j] = (__bf16)rval(kb * 32 + fq * 8 + j, (w * CTW + c) * 16 + fr);
    };
    fill();
  }
  if (trc_ && tid == 0) trc_[9] = (unsigned long long)(local + 1);  // step 0, slot 9
  // Self-tagged hand-off (fp32 partials, XCD-local slot, ring of two step
  // images set to tag 1 before the launch): the producer's partial-dh words
  // carry ((step >> 1) & 1) in their LSB, the consumers re-load a chunk until
  // all its words carry the step's tag.  No per-step drain, signal barrier,
  // flag store or flag poll -- the poll IS the payload load.  Ring safety as
  // before: a producer writes slot ks % 2 only after it has read every
  // consumer's step ks - 1 words, stored after that consumer's loads of step
  // ks - 2 had returned.  Nothing here rests on a wait at the end of a step
  // (STK has none): a consumer's loads of step ks - 2 are retired by its own
  // poll's vmcnt(0), every loading wave's, before the step's first barrier,
  // and its step ks - 1 words follow its second; a wave's stores to one slot,
  // two steps apart, have the poll between them retiring the older (HO4: a
  // wave that does not load has an explicit vmcnt(0) where the poll was).
  const bool dtag = !BF && p.dtag && local && p.ring == 2;
  // step t's DX rows for a streaming consumer on other XCDs, from the LDS
  // stage: written through (sc1) as whole 16-B chunks, 4 lanes per
  // contiguous 64-B run (4-B write-through stores per element cost ~8 us per
  // step); the next signal drains them, so they are complete at epoch t + 3
  auto e_sc1_store = [&](int tt) {
    constexpr int CPR = NW * U / 4;  // chunks per row
    // self-tagged (issued after the first barrier): the LAST 16 CPR threads,
    // i.e. the waves past the element waves when there are any, store while
    // the element waves do the cell
    // (IOA: from wave 4 on -- the 8 live rows' chunks stay on waves 4 and 5
    // for the GRU's 12 chunks a row too, off the IO waves)
    const int et = dtag ? tid - (IOA ? NTH / 2 : NTH - 16 * CPR) : tid;
    const int rn = et >= 0 ? et / CPR : 16, c = et - rn * CPR;
    if (rn < 16 && n0 + rn < nend) {
      const int q = (c * 4) / U, u = (c * 4) % U;
      const u32x4 v = *reinterpret_cast<const u32x4 *>(estg + rn * NW * U + c * 4);
      const int off = (int)(((long)(n0 + rn) * ldg + (long)d * NW * H + q * H + u0 + u) * 4);
      if constexpr (RST) {
        // (no streaming consumer: the same chunks with the plain policy)
        if (!p.e_sc1) {
          __builtin_amdgcn_raw_buffer_store_b128(v, rsrc(p.DX + (long)tt * N * ldg, (unsigned)(N * ldg * 4)), off, 0, 0);
          return;
        }
      }
      __builtin_amdgcn_raw_buffer_store_b128(v, rsrc(p.DX + (long)tt * N * ldg, (unsigned)(N * ldg * 4)), off, 0, 16);
    }
  };
  int t_prev = -1;
  int sl3 = 0;  // IOA: ks % 3, the operand slot of this step
  for (int k = T - 1; k >= 0 && !bad; k--) {
    const int t = d == 0 ? k : T - 1 - k;
    const int ks = T - 1 - k;  // steps done before this one
    REC_TRACE(ks, 0);
    if (ks > 0) {
      if (dtag) {
        // self-tagged: no flags; the poll below is the wait
      } else {
        wait_flags6(flag6(p, grp, d, 0, NWG), NWG, (unsigned)(ks + 1), p.err, bad, &bad_lds, p.poll_sleep);
      }
      REC_TRACE(ks, 1);
      REC_TRACE_W(ks, 16);
      const auto rs = rsrc(p.xch + (long)(p.ring ? (ks - 1) & 1 : ks - 1) * xstep, (unsigned)(xstep * 4));  // (ring: 2 images)
      floatx4 sm = floatx4{0.f, 0.f, 0.f, 0.f};
      if (bfp) {
        typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
        u32x2 v[PER];
        // unconditional (a dead row quad past the buffer: zeros), so that the
        // work below overlaps them
#pragma unroll
        for (int i = 0; i < PER; i++)
          v[i] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(
                     rs, crow_live ? (int)((coff + (long)i * NGRP * PSTR) * 4) : 0x7fff0000, 0, 16 /* sc1 */));
        if constexpr (PRE) {
          __builtin_amdgcn_sched_barrier(0);
          coef(k);  // while the hand-off loads are in flight
          __builtin_amdgcn_sched_barrier(0);
        } else {
          // bf16: the previous step's dGates rows / packed operands (its
          // cell's estg stage, complete since the MFMA phase's barrier) while
          // the hand-off loads are in flight, instead of after them
          __builtin_amdgcn_sched_barrier(0);
          e_store(t_prev);
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int i = 0; i < PER; i++) {
          const bf16x4 b = __builtin_bit_cast(bf16x4, v[i]);
#pragma unroll
          for (int j = 0; j < 4; j++) sm[j] += (float)b[j];
        }
      } else if (HO4 && !ho_wave) {
        // no hand-off loads, so no poll whose wait retires this wave's older
        // stores (partial dh two steps apart into one ring slot; waves 4, 5:
        // the write-through dGates rows behind the aggregated epoch): the
        // wait itself, in front of the step's first barrier, where this wave
        // idles for the loading waves anyway
        // IOA, waves 6 and 7: the exact wait.  Such a wave's queue, oldest
        // first, is F(ks - 2), S(ks - 2), F(ks - 1), S(ks - 1) -- F(j) the
        // NOP loads of the fetch it issued behind the first barrier of step j
        // (the operands of step j + 3), S(j) its 4 partial-dh stores of step
        // j -- and it needs F(ks - 2) landed (step ks + 1 reads that slot
        // behind this step's barriers) and S(ks - 2) retired (the ring of two
        // images): NOP + 4 stay in flight.  (The trace's stamps are stores of
        // these waves too: a traced run drains.)
        if (io_wave && !p.trace) io_wait();
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      } else {
        u32x4 v[PER];
        // unconditional loads (a dead row quad at an offset past the buffer:
        // the hardware returns zeros), so that the compiler counts them
        // exactly and the coefficients below overlap them
        auto hoff = [&](int i) { return crow_live ? (unsigned)((coff + (long)i * NGRP * PSTR) * 4) : 0x7fff0000u; };
#pragma unroll
        for (int i = 0; i < PER; i++) v[i] = ld_sc1(rs, hoff(i));
        if constexpr (PRE) {
          __builtin_amdgcn_sched_barrier(0);
          if constexpr (IOA) {
            // this step's operands, from the slot the IO waves filled (landed
            // before the last step's first barrier)
            if (has_e) {
              const float *os = ostg + sl3 * OSL + tid;
              cdy = os[0];
#pragma unroll
              for (int q = 0; q < NW; q++) cg[q] = os[(1 + q) * 8 * U];
              ca = os[(1 + NW) * 8 * U];
              cap_ld = os[(2 + NW) * 8 * U];
            }
          }
          if (!STK || has_e) coef(k);  // while the hand-off loads are in flight
          // (pinned here: IR passes had sunk the coefficients past the loads' wait)
#pragma unroll
          for (int q = 0; q < 6; q++) asm volatile("" : "+v"(kc[q]));
          __builtin_amdgcn_sched_barrier(0);
        }
        if (dtag) {
          // every word of step ks - 1 carries tag ((ks - 1) >> 1) & 1 in its
          // LSB; a chunk still holding step ks - 3's words (the other tag) is
          // loaded again.  4-B words are single-copy atomic, so a 16-B load
          // that tears between the two steps is caught word by word.
          const unsigned want = (unsigned)((ks - 1) >> 1) & 1u;
          auto ready = [&]() {
            unsigned bad4 = 0u;
#pragma unroll
            for (int i = 0; i < PER; i++) bad4 |= (v[i][0] ^ want) | (v[i][1] ^ want) | (v[i][2] ^ want) | (v[i][3] ^ want);
            return !crow_live || (bad4 & 1u) == 0u;
          };
          int spins = 0;
          while (!__all(ready())) {  // (not all there yet: the wave loads all its chunks again)
            if (++spins > kSpinLimit ||
                ((spins & 255) == 0 &&
                 __builtin_amdgcn_readfirstlane(__hip_atomic_load(p.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)))) {
              bad = 1;
              if (lane == 0) bad_lds = 1;
              break;
            }
            if (p.poll_sleep) __builtin_amdgcn_s_sleep(1);
            asm volatile("" ::: "memory");
#pragma unroll
            for (int i = 0; i < PER; i++) v[i] = ld_sc1(rs, hoff(i));
          }
        }
        sm = __builtin_bit_cast(floatx4, v[0]);
#pragma unroll
        for (int i = 1; i < PER; i++) sm += __builtin_bit_cast(floatx4, v[i]);
      }
      if (ho_wave) st4(red + (long)(pg * POS + pos) * 4, sm);
      REC_TRACE(ks, 2);
      REC_TRACE_W(ks, 24);
      // behind this step's hand-off loads: the write-through copies for the
      // streamed dx GEMM -- the previous step's dGates rows (staged in LDS)
      // and the epoch the last signal drained (step ks - 2's rows).  Issued
      // after the signal instead, they were still in flight at the next flag
      // poll, which waits for every older store (one vmcnt for loads and stores)
      // (self-tagged: after the barrier below, which orders it behind the
      // previous step's book() writes of estg -- no signal barrier in between)
      if ((RST || p.e_sc1) && !dtag) e_sc1_store(t_prev);
    }
    asm volatile("" ::: "memory");
    // behind the hand-off loads: next step's operands, last step's row-major dGates
    if (t_prev >= 0 && !(!PRE && bfp && ks > 0)) e_store(t_prev);
    if constexpr (!IOA) {  // (IOA: the IO waves fetch, behind the barrier)
      if (k > 0) prefetch(k - 1);
    }
    __syncthreads();
    REC_TRACE(ks, 8);
    // (STK: read here, looked at behind the cell -- the loop condition is its
    // only reader, and the LDS returns in order, so the element waves' red
    // reads do not wait for it)
    int bl = 0;
    if constexpr (STK) bl = bad_lds;
    else if (bad_lds) bad = 1;
    // self-tagged: every producer's words of step ks - 1 were stored behind
    // its second barrier of that step, which every wave reached after its
    // poll -- the hand-off loads' vmcnt(0), in order; HO4, waves 4..7: the
    // explicit vmcnt(0) in its place -- had retired the
    // write-through rows it issued in step ks - 2, those of step ks - 3
    // -> epoch ks (rows of step k out at epoch k + 3; no wait at the end of
    // a step is part of this);
    // flagged: its signal of step ks - 1 drained the rows of step ks - 2
    if (gflag && ks > 0 && tid == (GF4 ? NTH / 2 : 0))
      __hip_atomic_store(gflag, (unsigned)(dtag ? ks : ks + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (dtag && (RST || p.e_sc1) && ks > 0) e_sc1_store(t_prev);
    if constexpr (IOA) {
      // the operands of step ks + 3 into the slot step ks read in front of
      // this barrier: two step periods until the wait above needs them
      if (io_wave) io_fetch(sl3);
    }
    if (has_e) {
      float dhr = 0.f;
      if (ks > 0) {
        // all NGRP reads in flight before the first add (one LDS latency,
        // not NGRP), then the fixed-order sum
        float rr[NGRP];
#pragma unroll
        for (int gg = 0; gg < NGRP; gg++) rr[gg] = red[(long)(gg * POS + epos) * 4 + ereg];
        __builtin_amdgcn_sched_group_barrier(0x100, NGRP, 0);
#pragma unroll
        for (int gg = 0; gg < NGRP; gg++) dhr += rr[gg];
      }
      float dh = cdy + dhr;
      if constexpr (PRE) {
        if (MODE == kLstm) {
          const float dc = dh * kc[0] + carry;
          eg[0] = dc * kc[1];
          eg[1] = dc * kc[2];
          eg[2] = dc * kc[3];
          eg[3] = dh * kc[4];
          carry = dc * kc[5];
          if constexpr (STK) {
            // scalar products: packed with a broadcast dc, the unused half of
            // the pair fell on a register the prefetch is loading, and the
            // cell waited for the loads (vmcnt(0))
#pragma unroll
            for (int q = 0; q < NW; q++) asm volatile("" : "+v"(eg[q]));
          }
        } else {
          dh += carry;
          dxk[0] = dh * kc[0]; dxk[1] = dh * kc[1]; dxk[2] = dh * kc[2];
          eg[0] = dxk[0]; eg[1] = dxk[1]; eg[2] = dh * kc[3];
          carry = dh * kc[4];
        }
      } else if (MODE == kLstm) {
        const float ig = cg[0], fg = cg[1], gg = cg[2], og = cg[3];
        const float tc = ftanh(ca);
        const float dO = dh * tc;
        const float dc = dh * og * (1.f - tc * tc) + carry;
        eg[0] = dc * gg * ig * (1.f - ig);
        eg[1] = dc * cap_ld * fg * (1.f - fg);
        eg[2] = dc * ig * (1.f - gg * gg);
        eg[3] = dO * og * (1.f - og);
        carry = dc * fg;
      } else {
        dh += carry;
        const float r = cg[0], z = cg[1], nn = cg[2];
        const float dn = dh * (1.f - z), dz = dh * (cap_ld - nn);
        const float dpn = dn * (1.f - nn * nn);
        const float dpr = dpn * ca * r * (1.f - r);
        const float dpz = dz * z * (1.f - z);
        carry = dh * z;
        dxk[0] = dpr; dxk[1] = dpz; dxk[2] = dpn;
        eg[0] = dpr; eg[1] = dpz; eg[2] = dpn * r;
      }
      float m = 0.f;
#pragma unroll
      for (int q = 0; q < NW; q++) m = fmaxf(m, fabsf(eg[q]));
      if constexpr (!PRE) book();
      if constexpr (BF) {
#pragma unroll
        for (int q = 0; q < NW; q++) Ahi[en * AP + q * U + eu] = (__bf16)eg[q];
      } else {
        const int se = split_exp(group_maxU(m, U));
        // unit-major K: the element's NW gates are halves eu NW .. eu NW + NW - 1
        // of its row (STK: hi in row en < 8, lo in row en + 8)
        _Float16 hh[4], hl[4];
#pragma unroll
        for (int q = 0; q < 4; q++) hh[q] = hl[q] = (_Float16)0.f;
#pragma unroll
        for (int q = 0; q < NW; q++) split16(ldexpf(eg[q], se), hh[q], hl[q]);
        _Float16 *dhi = Ahi + en * AP + eu * NW;
        _Float16 *dlo = STK ? Ahi + (en + 8) * AP + eu * NW : Alo + en * AP + eu * NW;
        {
          if constexpr (NW == 4) {
            typedef _Float16 half4 __attribute__((ext_vector_type(4)));
            *reinterpret_cast<half4 *>(dhi) = half4{hh[0], hh[1], hh[2], hh[3]};
            *reinterpret_cast<half4 *>(dlo) = half4{hl[0], hl[1], hl[2], hl[3]};
          } else {
#pragma unroll
            for (int q = 0; q < NW; q++) {
              dhi[q] = hh[q];
              dlo[q] = hl[q];
            }
          }
        }
        if (eu == 0) rowexp[en] = se + sB;
      }
    }
    if constexpr (STK) {
      if (bl) bad = 1;
    }
    REC_TRACE(ks, 12);
    __syncthreads();
    REC_TRACE(ks, 3);
    if (STK && k > 0) {
      // partial dh of all units for the next step, stacked hi / lo: tile c's
      // four MFMAs, then -- while tile c + 1's run -- its fold, scaling, tag
      // and 16-B store, as one straight-line block per cache policy (the
      // store of a dead lane goes past the buffer's end and is dropped)
      const auto ro = rsrc(p.xch + (long)(p.ring ? ks & 1 : ks) * xstep, (unsigned)(xstep * 4));
      const long obase = (long)grp * xgrp + (long)(d * NWG + g) * PSTR;
      const unsigned tg = (unsigned)(ks >> 1) & 1u;
      const int e1 = -rowexp[fr & 7];
      AV ah[KB];
#pragma unroll
      for (int kb = 0; kb < KB; kb++) ah[kb] = *reinterpret_cast<const AV *>(Ahi + fr * AP + kb * 32 + fq * 8);
      auto phase = [&](auto aux_c) {
        constexpr int aux = decltype(aux_c)::value;
        floatx4 acc[CTW];
#pragma unroll
        for (int c = 0; c < CTW; c++) {
          acc[c] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int kb = 0; kb < KB; kb++) {  // the order of the interleaved version: hi, lo per k block
            acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bhi[c][kb], ah[kb], acc[c], 0, 0, 0);
            acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(blo[c][kb], ah[kb], acc[c], 0, 0, 0);
          }
        }
#pragma unroll
        for (int c = 0; c < CTW; c++) {
          floatx4 o;
#pragma unroll
          for (int i = 0; i < 4; i++) {
            float v = acc[c][i] + __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(acc[c][i]), 0x128, 0xF, 0xF, true));
            v = ldexpf(v, e1);
            o[i] = __uint_as_float((__float_as_uint(v) & ~1u) | tg);
          }
          const int slot = fq * 8 + (fr & 7);
          const int off = prow_live ? (int)((obase + ((long)(w * CTW + c) * 64 + slot) * LW) * 4) : 0x7ffffff0;
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), ro, off, 0, aux);
        }
        // pipeline: MFMAs of tiles 0 and 1, then per tile c the fold + store
        // of tile c - 1 ... interleaved with tile c + 1's MFMAs
        __builtin_amdgcn_sched_group_barrier(0x008, 2 * KB, 0);  // tile 0 (2 KB MFMAs a tile)
#pragma unroll
        for (int c = 1; c < CTW; c++) {
          __builtin_amdgcn_sched_group_barrier(0x008, KB, 0);  // tile c (first half)
          __builtin_amdgcn_sched_group_barrier(0x002, 12, 0);  // tile c - 1: fold, scale, tag
          __builtin_amdgcn_sched_group_barrier(0x008, KB, 0);  // tile c (second half)
          __builtin_amdgcn_sched_group_barrier(0x040, 1, 0);   // tile c - 1: store
        }
        __builtin_amdgcn_sched_group_barrier(0x002, 12, 0);  // last tile
        __builtin_amdgcn_sched_group_barrier(0x040, 1, 0);
      };
      if (local) phase(std::integral_constant<int, 0>{});
      else phase(std::integral_constant<int, 16>{});
    } else if (BF && k > 0 && bfp) {
      // bf16 with bf16 partials (configs[4]): the same pipeline -- tile c's KB
      // MFMAs, then its bf16 pack and 8-B store behind tile c + 1's
      const auto ro = rsrc(p.xch + (long)(p.ring ? ks & 1 : ks) * xstep, (unsigned)(xstep * 4));
      const long obase = (long)grp * xgrp + (long)(d * NWG + g) * PSTR;
      AV ah[KB];
#pragma unroll
      for (int kb = 0; kb < KB; kb++) ah[kb] = *reinterpret_cast<const AV *>(Ahi + fr * AP + kb * 32 + fq * 8);
      auto phase = [&](auto aux_c) {
        constexpr int aux = decltype(aux_c)::value;
        typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
        floatx4 acc[CTW];
#pragma unroll
        for (int c = 0; c < CTW; c++) {
          acc[c] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int kb = 0; kb < KB; kb++) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[kb], bhi[c][kb], acc[c], 0, 0, 0);
        }
#pragma unroll
        for (int c = 0; c < CTW; c++) {
          bf16x4 b;
#pragma unroll
          for (int i = 0; i < 4; i++) b[i] = (__bf16)acc[c][i];
          const int off = prow_live ? (int)((obase + ((long)(w * CTW + c) * 64 + lane) * LW) * 4) : 0x7ffffff0;
          __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, b), ro, off, 0, aux);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, KB, 0);  // tile 0
#pragma unroll
        for (int c = 1; c < CTW; c++) {
          __builtin_amdgcn_sched_group_barrier(0x008, KB, 0);  // tile c
          __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);   // tile c - 1: bf16 pack
          __builtin_amdgcn_sched_group_barrier(0x040, 1, 0);   // tile c - 1: store
        }
        __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);  // last tile
        __builtin_amdgcn_sched_group_barrier(0x040, 1, 0);
      };
      if (local) phase(std::integral_constant<int, 0>{});
      else phase(std::integral_constant<int, 16>{});
    } else if (k > 0) {  // partial dh of all units for the next step
      floatx4 acc[CTW];
#pragma unroll
      for (int c = 0; c < CTW; c++) acc[c] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kb = 0; kb < KB; kb++) {
        const AV ah = *reinterpret_cast<const AV *>(Ahi + fr * AP + kb * 32 + fq * 8);
        if constexpr (BF) {
#pragma unroll
          for (int c = 0; c < CTW; c++) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bhi[c][kb], acc[c], 0, 0, 0);
        } else if constexpr (STK) {
          // transposed: C^T[unit][row'] = R_slice^T dG^T, row' < 8 hi, >= 8 lo
          // (the R fragments as the A operand: same registers, A[unit][k])
#pragma unroll
          for (int c = 0; c < CTW; c++) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bhi[c][kb], ah, acc[c], 0, 0, 0);
#pragma unroll
          for (int c = 0; c < CTW; c++) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(blo[c][kb], ah, acc[c], 0, 0, 0);
        } else {
          const AV al = *reinterpret_cast<const AV *>(Alo + fr * AP + kb * 32 + fq * 8);
#pragma unroll
          for (int c = 0; c < CTW; c++) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bhi[c][kb], acc[c], 0, 0, 0);
#pragma unroll
          for (int c = 0; c < CTW; c++) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, blo[c][kb], acc[c], 0, 0, 0);
#pragma unroll
          for (int c = 0; c < CTW; c++) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bhi[c][kb], acc[c], 0, 0, 0);
        }
      }
      if constexpr (STK) {  // columns 8..15 (lo rows) onto 0..7: one DPP add (row_ror:8) per register
#pragma unroll
        for (int c = 0; c < CTW; c++)
#pragma unroll
          for (int i = 0; i < 4; i++)  // (mov_dpp with bound_ctrl: combined into one v_add_f32_dpp)
            acc[c][i] += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(acc[c][i]), 0x128, 0xF, 0xF, true));
      }
      int ex[4] = {0, 0, 0, 0};
      if constexpr (STK) {
        const int e1 = -rowexp[fr & 7];  // one row per lane
#pragma unroll
        for (int i = 0; i < 4; i++) ex[i] = e1;
      } else if constexpr (!BF) {
#pragma unroll
        for (int i = 0; i < 4; i++) ex[i] = -rowexp[fq * 4 + i];
      }
      // a ring of >= 2 images is safe: every workgroup is a consumer of every
      // producer, so before a producer writes slot ks % ring at step ks it saw
      // all flags of step ks - 1, i.e. every consumer had finished reading
      // that slot's previous contents (step ks - ring, read during ks - ring + 1)
      const auto ro = rsrc(p.xch + (long)(p.ring ? ks & 1 : ks) * xstep, (unsigned)(xstep * 4));
      const long obase = (long)grp * xgrp + (long)(d * NWG + g) * PSTR;
      // fp32 partials carry the step tag ((ks >> 1) & 1) in their LSB in every
      // mode (the self-tagged hand-off reads it; the others keep the same
      // arithmetic, so that pinned and unpinned runs stay bit-identical)
      const unsigned tg = (unsigned)(ks >> 1) & 1u;
#pragma unroll
      for (int c = 0; c < CTW; c++) {
        floatx4 o;
#pragma unroll
        for (int i = 0; i < 4; i++) {
          o[i] = BF ? acc[c][i] : ldexpf(acc[c][i], ex[i]);
          if (!bfp) o[i] = __uint_as_float((__float_as_uint(o[i]) & ~1u) | tg);
        }
        const int slot = STK ? (fq * 8 + (fr & 7)) : lane;  // STK: compact chunks of the 8 live columns
        const int off = (int)((obase + ((long)(w * CTW + c) * 64 + slot) * LW) * 4);
        // local: plain stores keep the lines in the XCD's shared L2, where the
        // consumers' sc1 loads find them; else write-through (sc1)
        if (!prow_live) {
        } else if (bfp) {
          typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
          bf16x4 b;
#pragma unroll
          for (int i = 0; i < 4; i++) b[i] = (__bf16)o[i];
          if (local) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, b), ro, off, 0, 0);
          else __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, b), ro, off, 0, 16);
        } else if (local) {
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), ro, off, 0, 0);
        } else {
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), ro, off, 0, 16);
        }
      }
    }
    // off the hand-off path (behind the partial-dh stores, during their
    // drain): bias and column-maximum bookkeeping, the dGates stage for the
    // next step's row writes (read after the publish barrier)
    if constexpr (PRE) {
      __builtin_amdgcn_sched_barrier(0);
      if (has_e) book();
    }
    REC_TRACE(ks, 7);
    if (!dtag) signal_epoch(myflag, (unsigned)(ks + 2), local);
    REC_TRACE(ks, 4);
    if constexpr (!STK) rotate();
    t_prev = t;
    sl3 = sl3 == 2 ? 0 : sl3 + 1;
    REC_TRACE(ks, 5);
  }
  if constexpr (IOA) {
    if (io_wave) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the fetches past the last step land
  }
  if (dtag) __syncthreads();  // the last step's book() writes of estg, before e_sc1_store reads them
  if (t_prev >= 0 && !bad) e_store(t_prev);
  if (!bad) {
    if ((RST || p.e_sc1) && t_prev >= 0) e_sc1_store(t_prev);
    signal_epoch(myflag, (unsigned)(T + 2), 0);  // the last step's rows are out
    if (gflag) {  // every producer's last rows are out
      wait_flags6(flag6(p, grp, d, 0, NWG), NWG, (unsigned)(T + 2), p.err, bad, &bad_lds, p.poll_sleep);
      if (!bad && tid == 0) __hip_atomic_store(gflag, (unsigned)(T + 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  // bias partial sums of this row group: reduce over its rows in a fixed
  // order through LDS; the host adds the groups in order
  float *bs = red;  // [2][16][U][NW] floats
  __syncthreads();
  if (has_r) {
#pragma unroll
    for (int q = 0; q < NW; q++) {
      const long b0 = ((long)en * U + eu) * NW + q;
      bs[b0] = live ? bsx[q] : 0.f;
      bs[(long)16 * U * NW + b0] = live ? ((MODE == kGru) ? bsh[q] : bsx[q]) : 0.f;
    }
  }
  __syncthreads();
  for (int q = tid; q < 2 * NW * U; q += NTH) {
    const int part = q / (NW * U), rem = q - part * NW * U, gt = rem / U, u = rem - gt * U;
    float s2 = 0.f;
    for (int r = 0; r < 16; r++) s2 += bs[(long)part * 16 * U * NW + ((long)r * U + u) * NW + gt];
    p.bias[(((long)grp * dirs + d) * 2 + part) * NW * H + gt * H + u0 + u] = s2;
  }
  if (p.cmax) {  // column maxima over all frames (this group's rows, through LDS; max over groups)
    constexpr int NP = MODE == kGru ? 2 : 1;
    __syncthreads();
    if (has_r) {
#pragma unroll
      for (int q = 0; q < NW; q++) {
        bs[((long)en * U + eu) * NW + q] = cmx[q];
        if (MODE == kGru) bs[(long)16 * U * NW + ((long)en * U + eu) * NW + q] = cme[q];
      }
    }
    __syncthreads();
    for (int q = tid; q < NP * NW * U; q += NTH) {
      const int part = q / (NW * U), rem = q - part * NW * U, gt = rem / U, u = rem - gt * U;
      float m2 = 0.f;
      for (int r = 0; r < 16; r++) m2 = fmaxf(m2, bs[(long)part * 16 * U * NW + ((long)r * U + u) * NW + gt]);
      unsigned *dst = p.cmax + (long)part * dirs * NW * H + (long)d * NW * H + gt * H + u0 + u;
      if (p.rg > 1) atomicMax(dst, __float_as_uint(m2));  // non-negative floats order as their bits
      else *dst = __float_as_uint(m2);
    }
  }
  if (bad && tid == 0) atomicOr(p.err, 1u);
}

struct Bwd6 {
  template <int MODE, int U, int H, int NTH, int P>
  static const void *get() {
    if constexpr ((P & 4) == 0) return reinterpret_cast<const void *>(rnn_bwd_rec6<MODE, U, H, NTH, P>);
    else throw std::logic_error("v6 recurrence: IO waves are a forward variant");
  }
};

}  // namespace

const void *rec6_bwd_kernel(int mode, int prec, int H, const V6Cfg &c) { return rec6_of<Bwd6>(mode, prec, H, c); }

}  // namespace kctc
